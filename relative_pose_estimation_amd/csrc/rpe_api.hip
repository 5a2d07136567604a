// rpe_api.hip -- host side of the C-ABI (include/rpe_amd.h): handle lifecycle,
// HBM workspace, host-built tables (pyramid geometry, resize coefficients,
// RANSAC subset stream and niters table) and stage orchestration on one HIP stream.
#include "rpe_internal.h"
#include "rpe_host.h"
#include <float.h>
#include <string.h>
#include <stdlib.h>

void rpe_orb_upload_constants(const signed char *disc, int n);

std::string g_create_err;       // what rpe_last_error(NULL) returns: the failure of the last rpe_create

// ---- argument heads: the checks several entry points share, each with its one message
int check_batch(rpe_handle *h, int B)
{
    if (B > h->cfg.max_batch) { h->err = "batch exceeds max_batch"; return RPE_ERR_CAPACITY; }
    return RPE_OK;
}
static int check_stream(rpe_handle *h, int F)
{
    if (F > h->n_img_cap || F - 1 > h->cfg.max_batch) { h->err = "stream longer than the handle capacity (frames <= 2*max_batch, pairs <= max_batch)"; return RPE_ERR_CAPACITY; }
    return RPE_OK;
}
int check_desc_counts(rpe_handle *h, const int32_t *n, int B)
{
    for (int i = 0; i < B; ++i) if (n[i] < 0 || n[i] > h->lay.kcap) { h->err = "descriptor count exceeds keypoint capacity"; return RPE_ERR_INVALID; }
    return RPE_OK;
}
// The byte-valued f32 descriptors of the L2 stage calls as the workspace holds them: u8 rows, the B sets of side 1 and then
// those of side 2, each of keypoint capacity; the counts are checked on the way
int l2_desc_bytes(rpe_handle *h, const float *h_desc1, const int32_t *n1, const float *h_desc2, const int32_t *n2, int B, std::vector<uint8_t> &u)
{
    const size_t dim = (size_t)h->desc_bytes;               // 128 (SIFT) or 32 (ORB descriptors under NORM_L2)
    const size_t per = (size_t)h->lay.kcap * dim;
    u.assign(2 * per * B, 0);
    for (int s = 0; s < 2; ++s) {
        const float *src = s ? h_desc2 : h_desc1; const int32_t *cn = s ? n2 : n1;
        for (int i = 0; i < B; ++i) {
            if (int rc = check_desc_counts(h, cn + i, 1)) return rc;
            for (size_t e = 0; e < (size_t)cn[i] * dim; ++e) {
                float v = src[(size_t)i * per + e];
                if (!(v >= 0.f && v <= 255.f) || v != (float)(int)v) { h->err = "NORM_L2 path expects byte-valued descriptors (SIFT's integer-valued 0..255 floats, or ORB bytes)"; return RPE_ERR_INVALID; }
                u[(size_t)s * per * B + (size_t)i * per + e] = (uint8_t)v;
            }
        }
    }
    return RPE_OK;
}
int check_match_counts(rpe_handle *h, const int32_t *m, int B)
{
    for (int i = 0; i < B; ++i) if (m[i] < 0 || m[i] > h->cfg.max_matches) { h->err = "match count exceeds max_matches"; return RPE_ERR_INVALID; }
    return RPE_OK;
}

// ---- the fetch: a device-to-host copy on the handle's stream for every piece the caller wants (dst != NULL), one wait
int fetch(rpe_handle *h, std::initializer_list<Copy> pieces)
{
    for (const Copy &f : pieces)
        if (f.dst) HIPCHK(h, hipMemcpyAsync(f.dst, f.src, f.bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RPE_OK;
}

// ---- the upload: a host-to-device copy on the handle's stream for every piece the caller gave (src != NULL) that has bytes; no wait
int upload(rpe_handle *h, std::initializer_list<Copy> pieces)
{
    for (const Copy &u : pieces)
        if (u.src && u.bytes > 0) HIPCHK(h, hipMemcpyAsync(u.dst, u.src, u.bytes, hipMemcpyHostToDevice, h->stream));
    return RPE_OK;
}
// Both sides of the B pairs of a stage call, pair p on the workspace slots (p, B + p): the keypoint counts, the 32-byte descriptors
int upload_counts(rpe_handle *h, const int32_t *n1, const int32_t *n2, int B)
{
    return upload(h, {{h->d_kp_count, n1, sizeof(int) * B}, {h->d_kp_count + B, n2, sizeof(int) * B}});
}
int upload_descriptors(rpe_handle *h, const uint8_t *h_desc1, const uint8_t *h_desc2, int B)
{
    const size_t side = (size_t)h->lay.kcap * 32 * B;
    return upload(h, {{h->d_desc, h_desc1, side}, {h->d_desc + side, h_desc2, side}});
}

// ---- the buffer set of a first-use feature, fitted to one call (the rule: rpe_internal.h)
int rpe_bufset_fit(rpe_handle *h, RpeBufSet &s, std::initializer_list<RpeBufPiece> pieces)
{
    RpeBufLayout need;
    for (const RpeBufPiece &pc : pieces) need.place(pc.bytes);
    if (need.total() > s.bytes) {
        uint8_t *old = s.block;
        if (old) HIPCHK(h, hipStreamSynchronize(h->stream));
        s = {};
        for (const RpeBufPiece &pc : pieces) *pc.p = nullptr;
        h->dev_allocs.erase(std::remove(h->dev_allocs.begin(), h->dev_allocs.end(), (void *)old), h->dev_allocs.end());
        if (old) HIPCHK(h, hipFree(old));
        if (int rc = dmalloc(h, &s.block, need.total())) return rc;
        s.bytes = need.total();
    }
    RpeBufLayout at;
    for (const RpeBufPiece &pc : pieces) {
        const size_t off = at.place(pc.bytes);
        *pc.p = off == RPE_BUF_NONE ? nullptr : s.block + off;
    }
    return RPE_OK;
}

int rpe_bufset_upload(rpe_handle *h, std::initializer_list<RpeBufPiece> pieces)
{
    for (const RpeBufPiece &pc : pieces)
        if (pc.src && pc.bytes > 0) HIPCHK(h, hipMemcpyAsync(*pc.p, pc.src, pc.bytes, hipMemcpyHostToDevice, h->stream));
    return RPE_OK;
}

// ---- argument heads of the calls behind a run: a parameter that must be finite and > 0, an array that must be finite
int check_positive(rpe_handle *h, const char *who, const char *name, double v)
{
    return std::isfinite(v) && v > 0. ? RPE_OK : rpe_invalid(h, who, (std::string(name) + " must be finite and > 0").c_str());
}
bool all_finite(const double *v, size_t n)
{
    bool fin = true;
    for (size_t i = 0; i < n; ++i) fin = fin && std::isfinite(v[i]);
    return fin;
}

static long long align_up(long long v, long long a) { return (v + a - 1) / a * a; }

extern "C" void rpe_default_config(rpe_config *c)
{
    memset(c, 0, sizeof(*c));
    c->abi_version = RPE_ABI_VERSION;
    c->device = 0;
    c->width = 640; c->height = 480;
    c->max_batch = 1;
    c->feature_method = RPE_FEATURE_ORB;   // pose_estimator.py:22
    c->norm_type = RPE_NORM_HAMMING;       // pose_estimator.py:23
    c->max_matches = 500;                  // pose_estimator.py:24
    c->nfeatures = 4000;                   // pose_estimator.py:25
    c->fast_threshold = 15;                // pose_estimator.py:89
    c->ransac_max_iters = 1000;
    c->ransac_prob = 0.999;                // pose_estimator.py:525
    c->ransac_threshold = 1.0;             // pose_estimator.py:526
    c->match_mode = RPE_MATCH_CROSSCHECK;  // pose_estimator.py:131 crossCheck=True
    c->match_ratio = 0.75;
    c->stl_runtime = RPE_STL_LIBSTDCXX;    // the reference's Linux cv2 wheels (Dockerfile: python:3.9-slim)
}

extern "C" int rpe_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" const char *rpe_last_error(const rpe_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }
extern "C" int rpe_keypoint_capacity(const rpe_handle *h) { return h ? h->lay.kcap : 0; }

// ORB pyramid geometry (orb.cpp): scale_l = (float)pow(1.1f, l), size cvRound(dim/scale),
// per-level quota from the geometric series, remainder to the last level.
static void build_layout(rpe_handle *h)
{
    RpeDeviceLayout &L = h->lay;
    const int W = h->cfg.width, H = h->cfg.height;
    // SIFT with nfeatures = 0 is cv2's SIFT_create() default: no retainBest; the arrays hold RPE_SIFT_UNCAPPED_CAPACITY keypoints
    const int nf = (h->cfg.feature_method == RPE_FEATURE_SIFT && h->cfg.nfeatures == 0) ? RPE_SIFT_UNCAPPED_CAPACITY : h->cfg.nfeatures;
    const double sf = (double)1.1f;
    long long off = 0;
    int coef = 0, cand = 0;
    for (int l = 0; l < RPE_NLEVELS; ++l) {
        RpeLevel &v = L.lv[l];
        v.scale = (float)pow(sf, (double)l);
        v.inv_scale = 1.0f / v.scale;                            // orb.cpp: Size sz(cvRound(image.cols * inv_scale), ...)
        v.w = cv_round((double)((float)W * v.inv_scale));
        v.h = cv_round((double)((float)H * v.inv_scale));
        v.pitch = (int)align_up(v.w, 16);
        v.off = off;
        off = align_up(off + (long long)v.pitch * v.h, 256);
        v.coef_off = coef;
        coef += 2 * (v.w + v.h);
    }
    L.stride = off;
    float factor = (float)(1.0 / sf);
    float nd = nf * (1 - factor) / (1 - (float)pow((double)factor, (double)RPE_NLEVELS));
    int sum = 0;
    for (int l = 0; l < RPE_NLEVELS - 1; ++l) {
        L.lv[l].quota = cv_round((double)nd);
        sum += L.lv[l].quota;
        nd *= factor;
    }
    L.lv[RPE_NLEVELS - 1].quota = nf - sum > 0 ? nf - sum : 0;
    int corner = 0;
    for (int l = 0; l < RPE_NLEVELS; ++l) {
        L.lv[l].ccap = rpe_corner_cap(L.lv[l].w, L.lv[l].h);     // raster corner list: clamp(w h / 64, 1024, 8192) entries
        L.lv[l].corner_off = corner;
        corner += L.lv[l].ccap;
        L.lv[l].kcap2 = 4 * L.lv[l].quota + 256;
        L.lv[l].cand_off = cand;
        cand += L.lv[l].kcap2;
    }
    L.corner_total = corner;
    L.cand_total = cand;
    L.stl = h->cfg.stl_runtime;
    L.kcap = nf + 64;
    L.fast_thr = h->cfg.fast_threshold;
}

// INTER_LINEAR_EXACT coefficients (resize.cpp interpolationLinear<ufixedpoint16>)
static void lin_coeffs(int src, int dst, int *ofs, int *a1)
{
    double inv_scale = (double)dst / (double)src;
    double scale = 1.0 / inv_scale;
    for (int d = 0; d < dst; ++d) {
        double f = scale * ((double)d + 0.5) - 0.5;
        int i = (int)floor(f);
        if (i >= 0 && src > 1) {
            if (i < src - 1) { ofs[d] = i; a1[d] = cv_round((f - (double)i) * 256.0); }
            else { ofs[d] = src - 1; a1[d] = 0; }
        } else { ofs[d] = 0; a1[d] = 0; }
    }
}

// cv::RNG (core/rand.cpp) MWC generator, used by RANSAC's getSubset
static inline uint32_t rng_next(uint64_t &st)
{
    st = (uint64_t)(uint32_t)st * 4164903690ULL + (uint32_t)(st >> 32);
    return (uint32_t)st;
}

static int build_tables(rpe_handle *h)
{
    const RpeDeviceLayout &L = h->lay;
    // tiles (also records each level's run of FAST tiles in the layout)
    std::vector<RpeTile> full, fast;
    for (int l = 0; l < RPE_NLEVELS; ++l) {
        const RpeLevel &v = L.lv[l];
        for (int y = 0; y < v.h; y += 64)
            for (int x = 0; x < v.pitch; x += 64) full.push_back({(short)l, (short)x, (short)y, 0});
        h->lay.lv[l].tile0 = (int)fast.size();
        if (v.w > 2 * RPE_EDGE && v.h > 2 * RPE_EDGE)
            // keypoints survive the border filter on [31, w-31) x [31, h-31) only; x origin dword aligned
            for (int y = RPE_EDGE; y < v.h - RPE_EDGE; y += FAST_TH)
                for (int x = FAST_TILE_X0; x < v.w - RPE_EDGE; x += 64) fast.push_back({(short)l, (short)x, (short)y, 0});
        h->lay.lv[l].ntile = (int)fast.size() - h->lay.lv[l].tile0;
        assert(h->lay.lv[l].ntile == rpe_fast_tiles(v.w, v.h));
    }
    // fast_nms_kernel loads pixels from (tx - 4, ty - 4) on and clamps only against the level's far edges
    for (const RpeTile &t : fast)
        if (t.tx < 4 || t.ty < 4) { h->err = "FAST tile origin below 4: the tile loads would start outside the level"; return RPE_ERR_INVALID; }
    h->n_tiles_full = (int)full.size(); h->n_tiles_fast = (int)fast.size();
    {
        int ntile[RPE_NLEVELS];
        for (int l = 0; l < RPE_NLEVELS; ++l) ntile[l] = L.lv[l].ntile;
        rpe_orb_groups(ntile, RPE_NLEVELS, RPE_ORB_GROUPS, h->orb_group);
    }
    DM(h, h->d_tiles_full, full.size());
    DM(h, h->d_tiles_fast, fast.size() ? fast.size() : 1);
    HIPCHK(h, hipMemcpy(h->d_tiles_full, full.data(), full.size() * sizeof(RpeTile), hipMemcpyHostToDevice));
    if (!fast.empty()) HIPCHK(h, hipMemcpy(h->d_tiles_fast, fast.data(), fast.size() * sizeof(RpeTile), hipMemcpyHostToDevice));
    // resize coefficients
    int ncoef = L.lv[RPE_NLEVELS - 1].coef_off + 2 * (L.lv[RPE_NLEVELS - 1].w + L.lv[RPE_NLEVELS - 1].h);
    std::vector<int> coef((size_t)ncoef, 0);
    for (int l = 1; l < RPE_NLEVELS; ++l) {
        const RpeLevel &S = L.lv[l - 1], &D = L.lv[l];
        int *xo = coef.data() + D.coef_off, *xa = xo + D.w, *yo = xa + D.w, *ya = yo + D.h;
        lin_coeffs(S.w, D.w, xo, xa);
        lin_coeffs(S.h, D.h, yo, ya);
    }
    // resize tiles (PYR_TW x PYR_TH destination pixels), levels 1..11: the origin of the source window (anchored at
    // floor(scale * tile origin), x aligned down to 16 B), the source rows the tile reads and its row-reuse mask.  The
    // kernel stages at most PYR_ROWS rows x (4 PYR_DW) bytes per tile and packs a source row's window byte offset into
    // PYR_YW_SHIFT bits: verify the tables fit both for every tile.
    {
        std::vector<RpePyrTile> pt;
        for (int l = 1; l < RPE_NLEVELS; ++l) {
            const RpeLevel &S = L.lv[l - 1], &D = L.lv[l];
            const int *xo = coef.data() + D.coef_off, *yo = xo + 2 * D.w;
            if ((long long)S.h * PYR_DW * 4 >= (1ll << PYR_YW_SHIFT)) { h->err = "pyramid level too tall for the packed row table"; return RPE_ERR_INVALID; }
            for (int x0 = 0; x0 < D.w; x0 += PYR_TW) {
                int a0 = ((int)(((long long)x0 * S.w) / D.w)) & ~15, xl = x0 + PYR_TW - 1 < D.w ? x0 + PYR_TW - 1 : D.w - 1;
                int hi = xo[xl] + 1 < S.w ? xo[xl] + 1 : S.w - 1;
                if (xo[x0] < a0 || hi - a0 >= PYR_DW * 4) { h->err = "pyramid footprint bound violated (x)"; return RPE_ERR_INVALID; }
            }
            h->pyr_tile_off[l] = (int)pt.size();
            for (int y0 = 0; y0 < D.h; y0 += PYR_TH) {
                const int s0 = (int)(((long long)y0 * S.h) / D.h), yl = y0 + PYR_TH - 1 < D.h ? y0 + PYR_TH - 1 : D.h - 1;
                // the last source row a destination row reads with a non-zero weight: rows 0 .. hi - s0 of the window are
                // loaded (all inside the level); the bottom row of a clamped top row (weight 0) is window row hi - s0 + 1,
                // which is read but need not hold anything, so it too has to lie inside the window
                const int hi = yo[yl] + 1 < S.h ? yo[yl] + 1 : S.h - 1;
                if (yo[y0] < s0 || hi - s0 >= PYR_ROWS || yo[yl] + 1 - s0 >= PYR_ROWS) { h->err = "pyramid footprint bound violated (y)"; return RPE_ERR_INVALID; }
                unsigned reuse = 0;
                for (int r = 1; y0 + r <= yl; ++r) reuse |= (unsigned)(yo[y0 + r] == yo[y0 + r - 1] + 1) << r;
                for (int x0 = 0; x0 < D.pitch; x0 += PYR_TW)
                    pt.push_back({(short)x0, (short)y0, (short)(((int)(((long long)x0 * S.w) / D.w)) & ~15), (short)s0,
                                  (unsigned short)(hi - s0 + 1), (unsigned short)reuse, 0});
            }
            h->pyr_tile_cnt[l] = (int)pt.size() - h->pyr_tile_off[l];
        }
        DM(h, h->d_pyr_tiles, pt.size() ? pt.size() : 1);
        if (!pt.empty()) HIPCHK(h, hipMemcpy(h->d_pyr_tiles, pt.data(), pt.size() * sizeof(RpePyrTile), hipMemcpyHostToDevice));
    }
    // device form: one dword per destination column / row.  x: offset | weight << 16 (offset < 65536, weight <= 256).
    // y: source row x window row pitch in bytes | weight << PYR_YW_SHIFT -- the row part is the same in every lane of a
    // tile, so the kernel reads its 16 entries with scalar loads and a lane adds one term to each (bound checked above).
    // Per level: [align128(w) packed x][align64(h) packed y], padded with the last entry, every run 16-B aligned: a lane
    // of the resize kernel fetches its 4 columns with one 16-B load, a wave its 16 rows with one scalar load, without clamps.
    {
        int dtotal = 0;
        for (int l = 1; l < RPE_NLEVELS; ++l) {
            h->lay.lv[l].dcoef_off = dtotal;
            dtotal += ((L.lv[l].w + 127) & ~127) + ((L.lv[l].h + 63) & ~63);
        }
        h->lay.lv[0].dcoef_off = 0;
        std::vector<int> packed((size_t)dtotal + 4, 0);
        for (int l = 1; l < RPE_NLEVELS; ++l) {
            const RpeLevel &D = L.lv[l];
            const int *xo = coef.data() + D.coef_off, *xa = xo + D.w, *yo = xa + D.w, *ya = yo + D.h;
            const int xw = (D.w + 127) & ~127, yh = (D.h + 63) & ~63;
            int *px = packed.data() + D.dcoef_off, *py = px + xw;
            for (int x = 0; x < xw; ++x) { const int k = x < D.w ? x : D.w - 1; px[x] = xo[k] | (xa[k] << 16); }
            for (int y = 0; y < yh; ++y) { const int k = y < D.h ? y : D.h - 1; py[y] = (int)((unsigned)(yo[k] * (PYR_DW * 4)) | ((unsigned)ya[k] << PYR_YW_SHIFT)); }
        }
        DM(h, h->d_coef, packed.size());
        HIPCHK(h, hipMemcpy(h->d_coef, packed.data(), sizeof(int) * packed.size(), hipMemcpyHostToDevice));
    }
    // intensity-centroid disc (orb.cpp umax table)
    {
        int umax[RPE_HALF_PATCH + 2];
        int v, v0, vmax = (int)floor(RPE_HALF_PATCH * sqrt(2.f) / 2 + 1);
        int vmin = (int)ceil(RPE_HALF_PATCH * sqrt(2.f) / 2);
        for (v = 0; v <= vmax; ++v) umax[v] = cv_round(sqrt((double)RPE_HALF_PATCH * RPE_HALF_PATCH - v * v));
        for (v = RPE_HALF_PATCH, v0 = 0; v >= vmin; --v) {
            while (umax[v0] == umax[v0 + 1]) ++v0;
            umax[v] = v0;
            ++v0;
        }
        std::vector<signed char> disc;
        for (int vv = -RPE_HALF_PATCH; vv <= RPE_HALF_PATCH; ++vv) {
            int d = umax[abs(vv)];
            for (int u = -d; u <= d; ++u) { disc.push_back((signed char)u); disc.push_back((signed char)vv); }
        }
        rpe_orb_upload_constants(disc.data(), (int)(disc.size() / 2));
    }
    // RANSAC subset stream per M (ptsetreg.cpp getSubset; RNG seeded (uint64)-1 per run)
    const int mm = h->cfg.max_matches, iters = h->cfg.ransac_max_iters;
    {
        std::vector<unsigned short> sub((size_t)(mm + 1) * iters * 5, 0);
        for (int M = 6; M <= mm; ++M) {
            uint64_t st = 0xFFFFFFFFFFFFFFFFULL;
            unsigned short *s = sub.data() + (size_t)M * iters * 5;
            for (int it = 0; it < iters; ++it, s += 5)
                for (int i = 0; i < 5; ++i) {
                    int v, dup;
                    do {
                        v = (int)(rng_next(st) % (uint32_t)M);
                        dup = 0;
                        for (int k = 0; k < i; ++k) if (s[k] == v) dup = 1;
                    } while (dup);
                    s[i] = (unsigned short)v;
                }
        }
        DM(h, h->d_subsets, sub.size());
        HIPCHK(h, hipMemcpy(h->d_subsets, sub.data(), sub.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
    }
    // RANSACUpdateNumIters(p, ep, 5, niters) terms per (M, goodCount)
    {
        size_t n = (size_t)(mm + 1) * (mm + 2) / 2;
        std::vector<double> den(n, 0.); std::vector<int> rnd(n, 0);
        double p = h->cfg.ransac_prob;
        p = p > 0. ? p : 0.; p = p < 1. ? p : 1.;
        double num0 = (1. - p) > DBL_MIN ? (1. - p) : DBL_MIN;
        h->nit_num = log(num0);
        for (int M = 1; M <= mm; ++M)
            for (int g = 0; g <= M; ++g) {
                size_t idx = (size_t)M * (M + 1) / 2 + g;
                double ep = (double)(M - g) / M;
                ep = ep > 0. ? ep : 0.; ep = ep < 1. ? ep : 1.;
                double denom = 1. - pow(1. - ep, 5);
                if (denom < DBL_MIN) { den[idx] = 0.; rnd[idx] = -1; continue; }
                denom = log(denom);
                den[idx] = denom;
                rnd[idx] = denom >= 0 ? 0 : cv_round(h->nit_num / denom);
            }
        DM(h, h->d_nit_denom, n); DM(h, h->d_nit_round, n);
        HIPCHK(h, hipMemcpy(h->d_nit_denom, den.data(), n * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(h->d_nit_round, rnd.data(), n * sizeof(int), hipMemcpyHostToDevice));
    }
    return RPE_OK;
}

// The result block of max_batch pairs: section k (R, t, inliers, status, n_matches) starts at off[k] and holds
// kRpeResultElem[k] bytes per pair
struct ResultBlock {
    size_t off[RPE_RESULT_SECTIONS], bytes = 0;
    explicit ResultBlock(const rpe_handle *h)
    {
        for (int k = 0; k < RPE_RESULT_SECTIONS; ++k) { off[k] = bytes; bytes += (size_t)h->cfg.max_batch * kRpeResultElem[k]; }
    }
};
static_assert(9 * sizeof(double) + 3 * sizeof(double) + 3 * sizeof(int) == RPE_RESULT_BYTES, "result sections");

// the first B pairs of the pinned mirror of a result block, section by section, into the caller's arrays (null: not wanted)
static void unpack_results(const rpe_handle *h, int B, double *R, double *t, int32_t *inliers, int32_t *n_matches, int32_t *status)
{
    const ResultBlock rb(h);
    void *dst[RPE_RESULT_SECTIONS] = {R, t, inliers, status, n_matches};
    for (int k = 0; k < RPE_RESULT_SECTIONS; ++k)
        if (dst[k]) memcpy(dst[k], h->h_resblk + rb.off[k], (size_t)B * kRpeResultElem[k]);
}

static int alloc_workspace(rpe_handle *h)
{
    const RpeDeviceLayout &L = h->lay;
    const size_t NI = (size_t)h->n_img_cap, B = (size_t)h->cfg.max_batch, mm = (size_t)h->cfg.max_matches;
    const size_t NIo = h->cfg.feature_method == RPE_FEATURE_SIFT ? 1 : NI;   // ORB pyramid buffers are unused by SIFT handles
    DM(h, h->d_pyr, NIo * L.stride); DM(h, h->d_bufA, L.stride);
    HIPCHK(h, hipMemset(h->d_bufA, 0, L.stride));
    HIPCHK(h, hipMemset(h->d_pyr, 0, NIo * L.stride));
    const size_t ntf = h->n_tiles_fast > 0 ? (size_t)h->n_tiles_fast : 1;
    DM(h, h->d_tile_cnt, NIo * ntf); DM(h, h->d_tile_list, NIo * ntf * RPE_FAST_TILE_CAP);
    HIPCHK(h, hipMemset(h->d_tile_cnt, 0, NIo * ntf * sizeof(int)));
    const size_t img = (size_t)h->cfg.width * h->cfg.height;
    DM(h, h->d_stage1, (B + 1) * img); DM(h, h->d_stage2, B * img);   // +1: a stream of max_batch pairs has max_batch + 1 frames
    DM(h, h->d_cand_xy, NI * L.cand_total); DM(h, h->d_cand_resp, NI * L.cand_total);
    DM(h, h->d_cand_count, NI * RPE_NLEVELS);
    DM(h, h->d_corner, NIo * L.corner_total); DM(h, h->d_corner_count, NI * RPE_NLEVELS); DM(h, h->d_kp_lvl_count, NI * RPE_NLEVELS);
    DM(h, h->d_kp_xy, NI * L.kcap); DM(h, h->d_kp_resp, NI * L.kcap); DM(h, h->d_kp_angle, NI * L.kcap);
    DM(h, h->d_kp_pt, NI * L.kcap); DM(h, h->d_kp_count, NI);
    DM(h, h->d_ovf, NI);
    HIPCHK(h, hipMemset(h->d_ovf, 0, NI * sizeof(unsigned)));
    DM(h, h->d_desc, NI * L.kcap * h->desc_bytes);
    HIPCHK(h, hipMemset(h->d_desc, 0, NI * L.kcap * h->desc_bytes));      // rpe_orb_detect_and_compute / rpe_sift_detect_and_compute copy whole rows of keypoint capacity out: rows no extraction ever wrote read as zero, not as what the allocator kept
    HIPCHK(h, hipMemset(h->d_kp_pt, 0, NI * L.kcap * sizeof(float2)));
    HIPCHK(h, hipMemset(h->d_kp_count, 0, NI * sizeof(int)));
    DM(h, h->d_m_q, B * mm); DM(h, h->d_m_t, B * mm); DM(h, h->d_m_d, B * mm);
    // results of a batch in ONE block [R 9B f64 | t 3B f64 | inliers B | status B | n_matches B]: rpe_fetch_results is one
    // device-to-host copy into pinned memory (five copies into pageable memory left the GPU idle for ~100 us per step)
    DM(h, h->d_resblk, (size_t)B * RPE_RESULT_BYTES);
    const ResultBlock rb(h);
    h->d_R = (double *)(h->d_resblk + rb.off[0]); h->d_t = (double *)(h->d_resblk + rb.off[1]);
    h->d_inliers = (int *)(h->d_resblk + rb.off[2]); h->d_status = (int *)(h->d_resblk + rb.off[3]); h->d_m_n = (int *)(h->d_resblk + rb.off[4]);
    HIPCHK(h, hipHostMalloc((void **)&h->h_resblk, (size_t)B * RPE_RESULT_BYTES));
    DM(h, h->d_pts1, B * mm); DM(h, h->d_pts2, B * mm);
    if (h->cfg.norm_type == RPE_NORM_L2) { DM(h, h->d_m_best, B * L.kcap); DM(h, h->d_m_best2, B * L.kcap); DM(h, h->d_m_norm, 2 * NI * L.kcap); }
    else {
        // the election words in HBM: for the batches that split (at most RPE_MATCH_SPLIT_PAIRS pairs), and for max_batch pairs
        // when the plan of either matcher keeps them there at that size too (beyond the split limit that is a matter of kcap
        // alone: every larger batch of this engine plans the same)
        size_t bs = std::min<size_t>(B, RPE_MATCH_SPLIT_PAIRS);
        for (int extra : {0, RPE_GUIDED_LDS_UINT4})
            if (rpe_hamming_plan(L.kcap, (int)B, extra).hbm) bs = B;
        DM(h, h->d_hm_best, bs * L.kcap); DM(h, h->d_hm_row, bs * L.kcap);
    }
    DM(h, h->d_n1, B * mm); DM(h, h->d_n2, B * mm);
    DM(h, h->d_rstate, B); DM(h, h->d_found, B);
    DM(h, h->d_models, B * RPE_RANSAC_MAXCHUNK * RPE_MAX_MODELS * 9);
    DM(h, h->d_hyp, B * (RPE_RANSAC_MAXCHUNK / 64) * 88 * 64);
    DM(h, h->d_nmodels, B * RPE_RANSAC_MAXCHUNK);
    DM(h, h->d_counts, B * RPE_RANSAC_MAXCHUNK * RPE_MAX_MODELS);
    DM(h, h->d_mask, B * mm);
    DM(h, h->d_E, B * 9);
    DM(h, h->d_K, 9);
    return RPE_OK;
}

// Every kernel that some legal handle launches with more than RPE_LDS_DEFAULT_BYTES of dynamic LDS gets its limit raised to
// its ceiling (the kernel files' lists) on the current device, before any launch or capture exists
static int raise_lds_limits(rpe_handle *h)
{
    for (auto list : {rpe_orb_lds_ceilings, rpe_match_lds_ceilings, rpe_similar_lds_ceilings, rpe_geom_lds_ceilings, rpe_link_lds_ceilings})
        for (const RpeLdsCeiling &c : list()) {
            const hipError_t e = hipFuncSetAttribute(c.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.bytes);
            if (e != hipSuccess) {
                h->err = std::string("raising the dynamic LDS limit of ") + c.name + " to " + std::to_string(c.bytes) + " bytes failed: " + hipGetErrorString(e);
                return RPE_ERR_HIP;
            }
        }
    return RPE_OK;
}

extern "C" int rpe_create(const rpe_config *cfg, rpe_handle **out)
{
    if (!cfg || !out) { g_create_err = "null argument"; return RPE_ERR_INVALID; }
    *out = nullptr;
    if (cfg->abi_version != RPE_ABI_VERSION) { g_create_err = "ABI version mismatch"; return RPE_ERR_INVALID; }
    const bool is_sift = cfg->feature_method == RPE_FEATURE_SIFT;
    if (cfg->feature_method != RPE_FEATURE_ORB && !is_sift) { g_create_err = "unknown feature method"; return RPE_ERR_INVALID; }
    if (cfg->norm_type != RPE_NORM_HAMMING && cfg->norm_type != RPE_NORM_L2) { g_create_err = "unknown norm type"; return RPE_ERR_INVALID; }
    if (is_sift && cfg->norm_type == RPE_NORM_HAMMING) {
        // cv2 builds this matcher but its match() rejects float descriptors (batchDistance: NORM_HAMMING needs CV_8U)
        g_create_err = "NORM_HAMMING needs 8-bit descriptors: SIFT descriptors are float (cv2 raises in match())"; return RPE_ERR_INVALID;
    }
    if (cfg->match_mode != RPE_MATCH_CROSSCHECK && cfg->match_mode != RPE_MATCH_RATIO) { g_create_err = "unknown match mode"; return RPE_ERR_INVALID; }
    if (cfg->norm_type == RPE_NORM_L2 && cfg->nfeatures > RPE_SIFT_UNCAPPED_CAPACITY) {
        // the L2 matcher sorts next_pow2(nfeatures + 64) 64-bit keys in LDS: 16384 keys = 128 KB of the CU's 160
        g_create_err = "NORM_L2: nfeatures must be <= 16320"; return RPE_ERR_INVALID;
    }
    if (cfg->stl_runtime != RPE_STL_LIBSTDCXX && cfg->stl_runtime != RPE_STL_MSVC) { g_create_err = "unknown stl_runtime"; return RPE_ERR_INVALID; }
    if (cfg->match_mode == RPE_MATCH_RATIO && !(cfg->match_ratio > 0. && cfg->match_ratio <= 1.)) { g_create_err = "match_ratio must be in (0, 1]"; return RPE_ERR_INVALID; }
    if (is_sift && (cfg->nfeatures > RPE_SIFT_UNCAPPED_CAPACITY || cfg->nfeatures < 0 || cfg->width > 4000 || cfg->height > 4000)) {
        g_create_err = "SIFT: nfeatures must be 0 (no cap: cv2's SIFT_create()) or a cap <= 16320, and the image <= 4000 px"; return RPE_ERR_INVALID;
    }
    if (cfg->width < 96 || cfg->height < 96 || cfg->width > RPE_MAX_IMAGE_DIM || cfg->height > RPE_MAX_IMAGE_DIM || cfg->max_batch < 1 ||
        (!is_sift && (cfg->nfeatures < 1 || cfg->nfeatures > RPE_ORB_MAX_FEATURES)) || cfg->max_matches < 5 || cfg->max_matches > RPE_MAX_MATCHES_LIMIT ||
        cfg->ransac_max_iters < 1 || cfg->ransac_max_iters > 4096 || cfg->fast_threshold < 1 || cfg->fast_threshold > 254) {
        g_create_err = "configuration out of supported range"; return RPE_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        g_create_err = "no HIP device available: the MI355X path has no CPU fallback"; return RPE_ERR_HIP;
    }
    if (cfg->device < 0 || cfg->device >= ndev) { g_create_err = "bad device ordinal"; return RPE_ERR_INVALID; }
    rpe_handle *h = new rpe_handle();
    h->cfg = *cfg;
    h->n_img_cap = 2 * cfg->max_batch;
    h->desc_bytes = is_sift ? 128 : 32;
    int rc = RPE_OK;
    do {
        if (hipSetDevice(cfg->device) != hipSuccess) { h->err = "hipSetDevice failed"; rc = RPE_ERR_HIP; break; }
        if ((rc = raise_lds_limits(h)) != RPE_OK) break;
        if (hipStreamCreate(&h->stream) != hipSuccess) { h->err = "hipStreamCreate failed"; rc = RPE_ERR_HIP; break; }
        build_layout(h);
        if ((rc = build_tables(h)) != RPE_OK) break;
        if ((rc = alloc_workspace(h)) != RPE_OK) break;
        if (is_sift && (rc = rpe_sift_create(h)) != RPE_OK) break;
        for (int i = 0; i <= RPE_STAGE_COUNT; ++i)
            if (hipEventCreate(&h->ev[i]) != hipSuccess) { h->err = "hipEventCreate failed"; rc = RPE_ERR_HIP; break; }
        if (rc != RPE_OK || is_sift) break;
        // the grouped schedule of run_orb: its side stream orders itself against the handle's stream through the events alone
        if (hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking) != hipSuccess) { h->err = "hipStreamCreateWithFlags failed"; rc = RPE_ERR_HIP; break; }
        bool ev_ok = hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) == hipSuccess;
        for (int g = 0; g < RPE_ORB_GROUPS && ev_ok; ++g) ev_ok = hipEventCreateWithFlags(&h->ev_fork[g], hipEventDisableTiming) == hipSuccess;
        if (!ev_ok) { h->err = "hipEventCreateWithFlags failed"; rc = RPE_ERR_HIP; break; }
    } while (0);
    if (rc != RPE_OK) { g_create_err = h->err; rpe_destroy(h); return rc; }
    *out = h;
    return RPE_OK;
}

static void frames_free(rpe_handle::FrameStore &fs)
{
    void *ptrs[] = {fs.d_desc, fs.d_kp_pt, fs.d_norm, fs.d_count, fs.d_ovf, fs.d_cam};
    for (void *p : ptrs) if (p) hipFree(p);
    fs = rpe_handle::FrameStore();
}

extern "C" void rpe_destroy(rpe_handle *h)
{
    if (!h) return;
    hipSetDevice(h->cfg.device);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->side_stream) { hipStreamSynchronize(h->side_stream); hipStreamDestroy(h->side_stream); }
    for (int g = 0; g < RPE_ORB_GROUPS; ++g) if (h->ev_fork[g]) hipEventDestroy(h->ev_fork[g]);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    rpe_sift_destroy(h);
    for (auto &g : h->graphs) { hipGraphExecDestroy(g.exec); hipGraphDestroy(g.graph); }
    for (void *p : h->dev_allocs) hipFree(p);
    if (h->h_resblk) hipHostFree(h->h_resblk);
    frames_free(h->fs);
    if (h->h_pairtab) hipHostFree(h->h_pairtab);
    for (int i = 0; i < RPE_TAB_RING; ++i) if (h->ev_tab[i]) hipEventDestroy(h->ev_tab[i]);
    for (void *p : h->user_allocs) hipFree(p);
    for (int i = 0; i <= RPE_STAGE_COUNT; ++i) if (h->ev[i]) hipEventDestroy(h->ev[i]);
    for (int c = 0; c < 8; ++c) if (h->ev_up[c]) hipEventDestroy(h->ev_up[c]);
    if (h->copy_stream) hipStreamDestroy(h->copy_stream);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

// ------------------------------------------------------------ device buffers
extern "C" int rpe_device_malloc(rpe_handle *h, size_t bytes, void **d_ptr)
{
    if (!h || !d_ptr) return rpe_invalid(h, "rpe_device_malloc");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMalloc(d_ptr, bytes));
    h->user_allocs.push_back(*d_ptr);
    return RPE_OK;
}
extern "C" int rpe_device_free(rpe_handle *h, void *d_ptr)
{
    if (!h) return rpe_invalid(h, "rpe_device_free");
    for (size_t i = 0; i < h->user_allocs.size(); ++i)
        if (h->user_allocs[i] == d_ptr) { h->user_allocs.erase(h->user_allocs.begin() + i); HIPCHK(h, hipFree(d_ptr)); return RPE_OK; }
    h->err = "rpe_device_free: unknown pointer";
    return RPE_ERR_INVALID;
}
extern "C" int rpe_host_alloc(rpe_handle *h, size_t bytes, void **h_ptr)
{
    if (!h || !h_ptr) return rpe_invalid(h, "rpe_host_alloc");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipHostMalloc(h_ptr, bytes, hipHostMallocDefault));
    return RPE_OK;
}
extern "C" int rpe_host_free(rpe_handle *h, void *h_ptr)
{
    if (!h) return rpe_invalid(h, "rpe_host_free");
    HIPCHK(h, hipHostFree(h_ptr));
    return RPE_OK;
}
extern "C" int rpe_host_register(rpe_handle *h, void *h_ptr, size_t bytes)
{
    if (!h || !h_ptr) return rpe_invalid(h, "rpe_host_register");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipHostRegister(h_ptr, bytes, hipHostRegisterDefault));
    return RPE_OK;
}
extern "C" int rpe_host_unregister(rpe_handle *h, void *h_ptr)
{
    if (!h || !h_ptr) return rpe_invalid(h, "rpe_host_unregister");
    HIPCHK(h, hipHostUnregister(h_ptr));
    return RPE_OK;
}
extern "C" int rpe_memcpy_h2d(rpe_handle *h, void *d, const void *s, size_t n)
{
    if (!h) return rpe_invalid(h, "rpe_memcpy_h2d");
    HIPCHK(h, hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RPE_OK;
}
extern "C" int rpe_memcpy_d2h(rpe_handle *h, void *d, const void *s, size_t n)
{
    if (!h) return rpe_invalid(h, "rpe_memcpy_d2h");
    HIPCHK(h, hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RPE_OK;
}
extern "C" int rpe_synchronize(rpe_handle *h)
{
    if (!h) return rpe_invalid(h, "rpe_synchronize");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RPE_OK;
}

// ------------------------------------------------------------- orchestration

// copies level 0 of every image into the pyramid buffer (device to device): when the level's pitch equals the image
// width, one strided copy per batch (an image is one "row" of it); otherwise one 2-D copy per image
static int load_level0(rpe_handle *h, const uint8_t *d_a, const uint8_t *d_b, int na, int nb)
{
    const int W = h->cfg.width, H = h->cfg.height;
    const RpeLevel &v = h->lay.lv[0];
    const size_t img = (size_t)W * H;
    if (v.pitch == W) {
        if (na) HIPCHK(h, hipMemcpy2DAsync(h->d_pyr + v.off, h->lay.stride, d_a, img, img, na, hipMemcpyDeviceToDevice, h->stream));
        if (nb) HIPCHK(h, hipMemcpy2DAsync(h->d_pyr + (size_t)na * h->lay.stride + v.off, h->lay.stride, d_b, img, img, nb,
                                           hipMemcpyDeviceToDevice, h->stream));
        return RPE_OK;
    }
    for (int i = 0; i < na + nb; ++i) {
        const uint8_t *src = i < na ? d_a + (size_t)i * img : d_b + (size_t)(i - na) * img;
        uint8_t *dst = h->d_pyr + (size_t)i * h->lay.stride + v.off;
        HIPCHK(h, hipMemcpy2DAsync(dst, v.pitch, src, W, W, H, hipMemcpyDeviceToDevice, h->stream));
    }
    return RPE_OK;
}

// Level 0 is the input itself: when its pitch equals the image width and the batches are 16-B aligned the kernels read
// it in place (rpe_level_base) -- the device-to-device copy into the pyramid buffer was 1.26 GB of HBM traffic and
// 0.22 ms per 1024 VGA pairs.  Other widths / unaligned batches take the copy.  Records the source of the na + nb images
// in the layout the kernels receive (a replayed graph holds it already; rpe_orb_debug_fetch reads it) and says which.
static bool set_level0_source(rpe_handle *h, const uint8_t *d_a, const uint8_t *d_b, int na, int nb)
{
    const bool direct = h->lay.lv[0].pitch == h->cfg.width && (((uintptr_t)d_a | (uintptr_t)(nb ? d_b : d_a)) & 15) == 0;
    h->lay.in_a = direct ? d_a : nullptr; h->lay.in_b = direct ? d_b : nullptr;
    h->lay.in_na = na; h->lay.in_img = h->cfg.width * h->cfg.height;
    h->level0_slots = na + nb;
    return direct;
}

static int run_orb(rpe_handle *h, const uint8_t *d_a, const uint8_t *d_b, int na, int nb)
{
    const int n = na + nb;
    MARK(h, RPE_STAGE_PYRAMID);
    HIPCHK(h, hipMemsetAsync(h->d_ovf, 0, sizeof(unsigned) * (size_t)n, h->stream));
    if (!set_level0_source(h, d_a, d_b, na, nb)) {
        int rc = load_level0(h, d_a, d_b, na, nb);
        if (rc) return rc;
    }
    // The selection chain of a level reads only what FAST wrote for that level, and FAST of a level only that level.  Small
    // batches (every captured one among them) build the pyramid, then run FAST and the chain once over all levels, one
    // kernel after the other.  From RPE_ORB_GROUP_MIN_IMAGES images on, the work is cut into level groups, largest levels
    // first (orb_groups.h), and the side stream takes what is bound by something else than its neighbour on the handle's
    // stream: FAST of group 0 (vector issue) as soon as the levels it reads exist, beside the resize of the levels above
    // them (HBM and latency); behind it the chain of group 0 and, behind each group's event, the chains of the groups
    // whose FAST runs on the handle's stream (latency), beside FAST of the groups after them.  The last group's chain
    // follows its FAST on the handle's stream, which then waits for the side stream.  The stage events stay on the handle's
    // stream and partition the step as before: `pyramid` spans the resize launches with FAST of group 0 beside the later
    // ones, `fast` the other groups' FAST and what the side stream ran beside them, `select`, `harris` and `keypoints` the
    // last group's chain, `keypoints` also the wait for the side stream and compact.
    const bool grouped = n >= RPE_ORB_GROUP_MIN_IMAGES;
    const int last = grouped ? RPE_ORB_GROUPS - 1 : 0;
    const RpeOrbGroup all = {0, RPE_NLEVELS, 0, h->n_tiles_fast};
    const int pyr_split = grouped ? std::max(h->orb_group[0].l1, 1) : RPE_NLEVELS;   // grouped: the levels group 0 reads come first
    hipError_t fe = hipSuccess;                   // the first failed fork / join call: what follows it stays on the handle's stream
    bool forked = false;
    rpe_launch_pyramid(h, n, 1, pyr_split);
    if (!grouped) MARK(h, RPE_STAGE_FAST);
    for (int g = 0; g < last; ++g) {
        const RpeOrbGroup &G = h->orb_group[g];
        if (g > 0) rpe_launch_fast(h, n, G.t0, G.nt, h->stream);
        hipStream_t s = h->stream;
        if (fe == hipSuccess) fe = hipEventRecord(h->ev_fork[g], h->stream);
        if (fe == hipSuccess) fe = hipStreamWaitEvent(h->side_stream, h->ev_fork[g], 0);
        if (fe == hipSuccess) { s = h->side_stream; forked = true; }
        if (g == 0) rpe_launch_fast(h, n, G.t0, G.nt, s);
        rpe_launch_raster_retain(h, n, G.l0, G.l1, s);
        rpe_launch_harris(h, n, G.l0, G.l1, s);
        rpe_launch_retain_harris(h, n, G.l0, G.l1, s);
        if (g == 0) { rpe_launch_pyramid(h, n, pyr_split, RPE_NLEVELS); MARK(h, RPE_STAGE_FAST); }
    }
    const RpeOrbGroup &G = grouped ? h->orb_group[last] : all;
    rpe_launch_fast(h, n, G.t0, G.nt, h->stream);
    MARK(h, RPE_STAGE_NMS);       // fused into fast_nms_kernel
    MARK(h, RPE_STAGE_SELECT);    rpe_launch_raster_retain(h, n, G.l0, G.l1, h->stream);
    MARK(h, RPE_STAGE_HARRIS);    rpe_launch_harris(h, n, G.l0, G.l1, h->stream);
    MARK(h, RPE_STAGE_KEYPOINTS); rpe_launch_retain_harris(h, n, G.l0, G.l1, h->stream);
    if (forked) {                 // whatever failed above, the side stream's work is joined before anything reads it
        hipError_t je = hipEventRecord(h->ev_join, h->side_stream);
        if (je == hipSuccess) je = hipStreamWaitEvent(h->stream, h->ev_join, 0);
        if (je != hipSuccess) { hipStreamSynchronize(h->side_stream); if (fe == hipSuccess) fe = je; }
    }
    HIPCHK(h, fe);
    rpe_launch_keypoints(h, n);
    MARK(h, RPE_STAGE_ANGLE);     rpe_launch_orient_describe(h, n);
    MARK(h, RPE_STAGE_BLUR);      // both fused into orient_describe_kernel (the whole-level blur runs on demand in rpe_orb_debug_fetch)
    MARK(h, RPE_STAGE_DESCRIBE);
    MARK(h, RPE_STAGE_MATCH);
    HIPCHK(h, hipGetLastError());
    return RPE_OK;
}

// keeps d_K current (re-uploaded only when the camera matrix changes)
int set_K(rpe_handle *h, const double K[9])
{
    if (h->K_valid && memcmp(h->K_last, K, sizeof(double) * 9) == 0) return RPE_OK;      // same camera as the last batch: already resident
    memcpy(h->K_last, K, sizeof(double) * 9);
    h->K_valid = false;
    if (int rc = upload(h, {{h->d_K, h->K_last, sizeof(double) * 9}})) return rc;
    h->K_valid = true;
    return RPE_OK;
}

// ---- the last run (RpeLastRun).  Every write to h->last is in the four functions below; every test of it in last_run_gate.
// An entry point that runs pairs calls last_run_begin with the run it is about to launch (a replayed graph included); one
// that overwrites workspace buffers without running pairs calls last_run_end.  A pair list hands over its slot arrays
// (kept as `tab`); a chunked host batch runs first and hands over the flag words it collected, image 1 of pair p at
// flags[p] and image 2 at flags[max_batch + p] (kept per pair as `ovf`).
static void last_run_begin(rpe_handle *h, RpeLastRun::Kind kind, const RpeRun &run, const int32_t *slot1 = nullptr,
                           const int32_t *slot2 = nullptr, const unsigned *flags = nullptr)
{
    RpeLastRun &l = h->last;
    l.kind = kind; l.pairs = run.pairs; l.run = run;
    l.tab.clear(); l.ovf.clear();
    for (int p = 0; kind == RpeLastRun::LIST && p < run.pairs; ++p) { l.tab.push_back(slot1[p]); l.tab.push_back(slot2[p]); }
    for (int p = 0; kind == RpeLastRun::CHUNKED && p < run.pairs; ++p) l.ovf.push_back(flags[p] | flags[h->cfg.max_batch + p]);
    l.per_match = kind != RpeLastRun::CHUNKED;      // a chunked batch leaves its last chunk's only
    l.structure = 0;
    h->ev_first = kind == RpeLastRun::LIST ? RPE_STAGE_MATCH : 0;
}

// The last run's claim on the per-match buffers ends (a stage call overwrites them, a failed launch sequence never filled
// them); images_too: on the per-image arrays and the device pair table as well (rpe_frames_put*), nothing is left to fetch
void last_run_end(rpe_handle *h, bool images_too)
{
    h->last.per_match = false;
    h->last.structure = 0;
    if (images_too) { h->last.kind = RpeLastRun::NONE; h->last.pairs = 0; }
}

// The frame store changed under a pair list.  resized (rpe_frames_reserve): the list's slot numbers mean nothing any more,
// its table goes; either way (rpe_frames_set_cameras too) a camera list read the store's camera records: its per-match
// results end here
static void last_run_store_changed(rpe_handle *h, bool resized)
{
    if (resized) h->last.tab.clear();
    if (h->last.run.cam.tab) last_run_end(h);
}

// the first B pairs of the last run: what the calls behind it launch on
RpeRun last_run_first(const rpe_handle *h, int B)
{
    RpeRun r = h->last.run;
    r.pairs = B;
    return r;
}

// Makes d_mask (status form), d_pose_mask and d_points current for the first B pairs of the last run: the two buffers on
// first use, the structure kernels (again: always; otherwise only when the run is not covered that far), the record
int last_run_structure(rpe_handle *h, int B, bool always)
{
    const size_t cap = (size_t)h->cfg.max_batch * h->cfg.max_matches;
    DM_ONCE(h, h->d_pose_mask, cap);
    DM_ONCE(h, h->d_points, cap * 3);
    if (!always && h->last.structure >= B) return RPE_OK;
    rpe_launch_structure(h, last_run_first(h, B));
    HIPCHK(h, hipGetLastError());
    h->last.structure = std::max(h->last.structure, B);
    return RPE_OK;
}

// The gate of the calls behind the last run: the only code that refuses one for the state of h->last.  n: pairs asked for.
//
// | call                                                  | NEED_UNCHUNKED        | NEED_PER_MATCH | NEED_COUNT (n <= pairs)    | NEED_TABLE (a list keeps 2*n entries) |
// |-------------------------------------------------------|-----------------------|----------------|----------------------------|---------------------------------------|
// | rpe_fetch_overflow                                    | no (served from ovf)  | no             | yes                        | yes, n = n_pairs                      |
// | rpe_fetch_matched_points, rpe_fetch_match_indices     | yes                   | no             | no                         | no                                    |
// | rpe_fetch_structure, rpe_refine_poses                 | yes                   | yes            | yes                        | no                                    |
// | rpe_scale_links, rpe_link_poses, rpe_link_bundles     | yes                   | yes            | no (checks its links' own) | yes, n = the run's pairs              |
// | rpe_guided_matches(_l2), rpe_pair_homographies        | yes                   | yes            | yes                        | yes, n = B                            |
// | rpe_build_tracks                                      | yes                   | yes            | no (runs over all pairs)   | yes, n = the run's pairs              |
//
// Tested in this order, so a state gives one message whatever the call.  Two tests stay with their callers:
// the link calls' and rpe_build_tracks' "the pairs of a batch share no frame" and rpe_fetch_overflow's slot range.
int last_run_gate(rpe_handle *h, const char *who, int n, unsigned needs)
{
    const RpeLastRun &l = h->last;
    const char *why = nullptr;
    if ((needs & NEED_UNCHUNKED) && l.kind == RpeLastRun::CHUNKED)
        why = ": the last host batch ran in chunks: what a run leaves per match is kept for unchunked and device-resident batches (rpe_estimate_batch_device) only";
    else if ((needs & NEED_PER_MATCH) && !l.per_match) why = ": no batch or stream since the last stage-API call (it overwrote the per-match buffers)";
    else if ((needs & NEED_COUNT) && n > l.pairs) why = ": more pairs than the last batch had";
    else if ((needs & NEED_TABLE) && l.kind == RpeLastRun::LIST && l.tab.size() < (size_t)2 * n) why = ": the frame store was resized since the pair list";
    if (why) { h->err = std::string(who) + why; return RPE_ERR_INVALID; }
    return RPE_OK;
}

extern "C" int rpe_last_run_pairs(const rpe_handle *h) { return h ? h->last.pairs : 0; }

// match -> RANSAC -> pose of run r: the tail of the image paths and the whole of a pair list
static int run_tail(rpe_handle *h, const RpeRun &r)
{
    if (h->cfg.norm_type == RPE_NORM_L2) rpe_launch_match_l2(h, r);
    else rpe_launch_match(h, r);
    MARK(h, RPE_STAGE_RANSAC);
    rpe_launch_ransac(h, r, false);
    MARK(h, RPE_STAGE_POSE);
    rpe_launch_pose(h, r, true);
    if (h->profiling) { hipEventRecord(h->ev[RPE_STAGE_COUNT], h->stream); h->ev_valid = true; }
    HIPCHK(h, hipGetLastError());
    return RPE_OK;
}

// feature extraction of na + nb images into the workspace slots [0, na + nb), then the tail of run r over them
static int run_images(rpe_handle *h, const uint8_t *d_a, const uint8_t *d_b, int na, int nb, const RpeRun &r)
{
    last_run_begin(h, RpeLastRun::RULE, r);
    int rc;
    if (h->cfg.feature_method == RPE_FEATURE_SIFT) {
        rc = rpe_sift_run(h, d_a, d_b, na, nb);             // records PYRAMID .. DESCRIBE
        MARK(h, RPE_STAGE_MATCH);
    } else
        rc = run_orb(h, d_a, d_b, na, nb);
    if (rc == RPE_OK) rc = run_tail(h, r);
    if (rc != RPE_OK) last_run_end(h);
    return rc;
}

extern "C" int rpe_enqueue_batch_device(rpe_handle *h, const uint8_t *d_imgs1, const uint8_t *d_imgs2, int B, const double K[9])
{
    if (!h || !d_imgs1 || !d_imgs2 || !K || B < 1) return rpe_invalid(h, "rpe_enqueue_batch_device");
    if (int rc = check_batch(h, B)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = set_K(h, K);
    if (rc) return rc;
    // Small batches are launch-bound on the HOST (one pair: ~50 launches for 0.6 ms of GPU work): the sequence is captured
    // once per (input buffers, B) and replayed as a hipGraph.  Everything in it is stream-ordered kernels and memsets whose
    // arguments depend only on the handle, the two buffers and B; K travels outside (set_K above).  Not while profiling (the
    // stage events are host-side records) and only for ORB (rpe_sift_run has no host sync either, but its sequence is not
    // captured: the condition below is the ORB one), RPE_NO_GRAPH=1 turns it off.  No launcher in the sequence reads the
    // environment, so a cached graph cannot freeze a switch.
    static const bool no_graph = getenv("RPE_NO_GRAPH") != nullptr;
    if (B > RPE_GRAPH_MAX_PAIRS || h->profiling || h->cfg.feature_method != RPE_FEATURE_ORB || no_graph)
        return run_images(h, d_imgs1, d_imgs2, B, B, rpe_run_batch(h, B));
    for (auto &g : h->graphs)
        if (g.a == d_imgs1 && g.b == d_imgs2 && g.B == B) {
            last_run_begin(h, RpeLastRun::RULE, rpe_run_batch(h, B));
            set_level0_source(h, d_imgs1, d_imgs2, B, B);
            HIPCHK(h, hipGraphLaunch(g.exec, h->stream));
            return RPE_OK;
        }
    rpe_handle::GraphEntry e{d_imgs1, d_imgs2, B, nullptr, nullptr};
    if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        return run_images(h, d_imgs1, d_imgs2, B, B, rpe_run_batch(h, B));
    }
    rc = run_images(h, d_imgs1, d_imgs2, B, B, rpe_run_batch(h, B));
    const hipError_t ce = hipStreamEndCapture(h->stream, &e.graph);
    if (rc != RPE_OK || ce != hipSuccess || !e.graph || hipGraphInstantiate(&e.exec, e.graph, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (e.graph) hipGraphDestroy(e.graph);
        return rc != RPE_OK ? rc : run_images(h, d_imgs1, d_imgs2, B, B, rpe_run_batch(h, B));       // capture unavailable: plain launches
    }
    if (h->graphs.size() >= 4) {                                                    // a handful of (buffers, B) combinations at most
        hipGraphExecDestroy(h->graphs.front().exec); hipGraphDestroy(h->graphs.front().graph);
        h->graphs.erase(h->graphs.begin());
    }
    h->graphs.push_back(e);
    HIPCHK(h, hipGraphLaunch(e.exec, h->stream));
    return RPE_OK;
}

// Consecutive-frame stream (reference batch_processor.py:71-109): F frames -> F-1
// pairs (i, i+1).  Features are extracted ONCE per frame (the reference extracts every interior
// frame twice, batch_processor.py:79,92); pair p reads image slots p and p+1.
extern "C" int rpe_enqueue_stream_device(rpe_handle *h, const uint8_t *d_frames, int F, const double K[9])
{
    if (!h || !d_frames || !K || F < 2) return rpe_invalid(h, "rpe_enqueue_stream_device");
    if (int rc = check_stream(h, F)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = set_K(h, K);
    if (rc) return rc;
    return run_images(h, d_frames, d_frames, F, 0, rpe_run_stream(h, F - 1));
}

extern "C" int rpe_estimate_stream(rpe_handle *h, const uint8_t *h_frames, int F, const double K[9],
                                   double *R, double *t, int32_t *inliers, int32_t *n_matches, int32_t *status)
{
    if (!h || !h_frames || F < 2) return rpe_invalid(h, "rpe_estimate_stream");
    if (int rc = check_stream(h, F)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t img = (size_t)h->cfg.width * h->cfg.height;
    // d_stage1 holds max_batch + 1 frames: every legal stream fits the persistent staging buffer
    int rc = upload(h, {{h->d_stage1, h_frames, img * F}});
    if (!rc) rc = rpe_enqueue_stream_device(h, h->d_stage1, F, K);
    if (rc) return rc;
    return rpe_fetch_results(h, F - 1, R, t, inliers, n_matches, status);
}

// ---------------------------------------------------------------- image ingest
// cv2.cvtColor(BGR2GRAY) (reference src/utils/image_loader.py:27-28), 8-bit path of OpenCV's color_rgb:
// (B*3735 + G*19235 + R*9798 + (1 << 14)) >> 15.  HBM-bound streaming kernel: a lane turns 16 pixels
// (three 16-B loads) into one 16-B store; 4 algorithmic bytes per pixel.
__global__ __launch_bounds__(256) void bgr_to_gray_kernel(const uint8_t *__restrict__ bgr, uint8_t *__restrict__ gray, size_t n_pixels,
                                                          unsigned w0, unsigned w1, unsigned w2)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;        // group of 16 pixels
    const size_t p0 = g * 16;
    if (p0 >= n_pixels) return;
    if (p0 + 16 <= n_pixels) {
        const uint4 *src = (const uint4 *)(bgr + p0 * 3);
        const uint4 a = src[0], b = src[1], c = src[2];
        const unsigned wd[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
        unsigned out[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int o = 3 * i;
            const unsigned c0 = (wd[o >> 2] >> (8 * (o & 3))) & 255u;
            const unsigned c1 = (wd[(o + 1) >> 2] >> (8 * ((o + 1) & 3))) & 255u;
            const unsigned c2 = (wd[(o + 2) >> 2] >> (8 * ((o + 2) & 3))) & 255u;
            out[i >> 2] |= ((c0 * w0 + c1 * w1 + c2 * w2 + 16384u) >> 15) << (8 * (i & 3));
        }
        *(uint4 *)(gray + p0) = make_uint4(out[0], out[1], out[2], out[3]);
    } else {
        for (size_t p = p0; p < n_pixels; ++p)
            gray[p] = (uint8_t)((bgr[3 * p] * w0 + bgr[3 * p + 1] * w1 + bgr[3 * p + 2] * w2 + 16384u) >> 15);
    }
}

extern "C" int rpe_bgr_to_gray_device(rpe_handle *h, const uint8_t *d_bgr, size_t n_pixels, int order, uint8_t *d_gray)
{
    if (!h || !d_bgr || !d_gray || (order != RPE_ORDER_BGR && order != RPE_ORDER_RGB)) return rpe_invalid(h, "rpe_bgr_to_gray_device");
    if (((uintptr_t)d_bgr | (uintptr_t)d_gray) & 15) { h->err = "rpe_bgr_to_gray_device: buffers must be 16-byte aligned"; return RPE_ERR_INVALID; }
    if (n_pixels == 0) return RPE_OK;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const unsigned wb = 3735u, wg = 19235u, wr = 9798u;
    const size_t groups = (n_pixels + 15) / 16;
    hipLaunchKernelGGL(bgr_to_gray_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, h->stream, d_bgr, d_gray, n_pixels,
                       order == RPE_ORDER_BGR ? wb : wr, wg, order == RPE_ORDER_BGR ? wr : wb);
    HIPCHK(h, hipGetLastError());
    return RPE_OK;
}

extern "C" int rpe_bgr_to_gray(rpe_handle *h, const uint8_t *h_bgr, size_t n_pixels, int order, uint8_t *h_gray)
{
    if (!h || !h_bgr || !h_gray) return rpe_invalid(h, "rpe_bgr_to_gray");
    if (n_pixels == 0) return RPE_OK;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    void *d_in = nullptr, *d_out = nullptr;
    HIPCHK(h, hipMalloc(&d_in, n_pixels * 3));
    if (hipMalloc(&d_out, n_pixels) != hipSuccess) { hipFree(d_in); h->err = "hipMalloc failed"; return RPE_ERR_HIP; }
    int rc = RPE_OK;                                         // of the conversion, which leaves its own text
    bool copied = hipMemcpyAsync(d_in, h_bgr, n_pixels * 3, hipMemcpyHostToDevice, h->stream) == hipSuccess;
    if (copied) rc = rpe_bgr_to_gray_device(h, (const uint8_t *)d_in, n_pixels, order, (uint8_t *)d_out);
    if (copied && !rc) copied = hipMemcpyAsync(h_gray, d_out, n_pixels, hipMemcpyDeviceToHost, h->stream) == hipSuccess;
    copied = (hipStreamSynchronize(h->stream) == hipSuccess) && copied;
    hipFree(d_in); hipFree(d_out);
    if (!rc && !copied) { h->err = "rpe_bgr_to_gray: HIP failure"; rc = RPE_ERR_HIP; }
    return rc;
}

extern "C" int rpe_fetch_results(rpe_handle *h, int B, double *R, double *t, int32_t *inliers, int32_t *n_matches, int32_t *status)
{
    if (!h || B < 1 || B > h->cfg.max_batch) return rpe_invalid(h, "rpe_fetch_results");
    const ResultBlock rb(h);
    // the used part of every section when the batch is small, the whole block in one piece otherwise
    if ((size_t)B * 4 < (size_t)h->cfg.max_batch) {
        for (int k = 0; k < RPE_RESULT_SECTIONS; ++k)
            HIPCHK(h, hipMemcpyAsync(h->h_resblk + rb.off[k], h->d_resblk + rb.off[k], (size_t)B * kRpeResultElem[k], hipMemcpyDeviceToHost, h->stream));
    } else {
        HIPCHK(h, hipMemcpyAsync(h->h_resblk, h->d_resblk, rb.bytes, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    unpack_results(h, B, R, t, inliers, n_matches, status);
    return RPE_OK;
}

extern "C" int rpe_fetch_overflow(rpe_handle *h, int n_pairs, uint32_t *flags)
{
    if (!h || !flags || n_pairs < 1 || n_pairs > h->cfg.max_batch) return rpe_invalid(h, "rpe_fetch_overflow");
    int rc = last_run_gate(h, "rpe_fetch_overflow", n_pairs, NEED_COUNT | NEED_TABLE);
    if (rc) return rc;
    const RpeLastRun &l = h->last;
    if (l.kind == RpeLastRun::CHUNKED) {
        // a chunked host batch reuses the per-image flag words chunk after chunk: they were collected per pair as the chunks finished
        memcpy(flags, l.ovf.data(), sizeof(uint32_t) * (size_t)n_pairs);
        return RPE_OK;
    }
    if (l.kind == RpeLastRun::LIST) {
        // a pair list: the flags live with the frames (a put since then ended the run, a resize of the store emptied its table)
        int lo = l.tab[0], hi = lo;
        for (int i = 0; i < 2 * n_pairs; ++i) { lo = std::min(lo, l.tab[i]); hi = std::max(hi, l.tab[i]); }
        if (lo < 0 || hi >= h->fs.cap) { h->err = "rpe_fetch_overflow: the pair list names slots outside the store"; return RPE_ERR_INVALID; }
        std::vector<unsigned> ov((size_t)(hi - lo + 1));       // the slots the list names, not the whole store
        if ((rc = fetch(h, {{ov.data(), h->fs.d_ovf + lo, sizeof(unsigned) * ov.size()}})) != RPE_OK) return rc;
        for (int p = 0; p < n_pairs; ++p) flags[p] = ov[(size_t)(l.tab[2 * p] - lo)] | ov[(size_t)(l.tab[2 * p + 1] - lo)];
        return RPE_OK;
    }
    const int img2_base = l.run.feat.img2_base, nimg = img2_base + n_pairs;
    std::vector<unsigned> ov((size_t)nimg);
    if ((rc = fetch(h, {{ov.data(), h->d_ovf, sizeof(unsigned) * (size_t)nimg}})) != RPE_OK) return rc;
    for (int p = 0; p < n_pairs; ++p) flags[p] = ov[p] | ov[img2_base + p];
    return RPE_OK;
}

extern "C" int rpe_estimate_batch_device(rpe_handle *h, const uint8_t *d_imgs1, const uint8_t *d_imgs2, int B, const double K[9],
                                         double *R, double *t, int32_t *inliers, int32_t *n_matches, int32_t *status)
{
    int rc = rpe_enqueue_batch_device(h, d_imgs1, d_imgs2, B, K);
    if (rc) return rc;
    return rpe_fetch_results(h, B, R, t, inliers, n_matches, status);
}

// Large host batches run in chunks (rpe_estimate_batch)
static bool batch_is_chunked(const rpe_handle *h, int B)
{
    return B >= 512 && (size_t)h->cfg.width * h->cfg.height * (size_t)B >= ((size_t)64 << 20);
}

// n host images into the staging buffers, the first max_batch into d_stage1 and the rest into d_stage2: the (d_a, d_b, na, nb)
// an extraction over workspace slots [0, n) takes
static int stage_images(rpe_handle *h, const uint8_t *h_imgs, int n, int &na, int &nb)
{
    const size_t img = (size_t)h->cfg.width * h->cfg.height;
    na = n < h->cfg.max_batch ? n : h->cfg.max_batch; nb = n - na;
    return upload(h, {{h->d_stage1, h_imgs, img * na}, {h->d_stage2, h_imgs + img * na, img * nb}});
}

extern "C" int rpe_estimate_batch(rpe_handle *h, const uint8_t *h_imgs1, const uint8_t *h_imgs2, int B, const double K[9],
                                  double *R, double *t, int32_t *inliers, int32_t *n_matches, int32_t *status)
{
    if (!h || !h_imgs1 || !h_imgs2 || B < 1) return rpe_invalid(h, "rpe_estimate_batch");
    if (int rc = check_batch(h, B)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t img = (size_t)h->cfg.width * h->cfg.height;
    // Large host batches run in chunks: all uploads are queued on a copy stream, chunk c's kernels wait for its
    // 'resident' event only, so the PCIe transfer of the later chunks hides behind the kernels of the earlier ones
    // (1024 VGA pairs: 629 MB = 12 ms of copy in front of 16 ms of kernels when done in one piece).
    const int nchunks = batch_is_chunked(h, B) ? 4 : 1;    // 2/3/4/6/8 chunks measured: 23.1/22.4/22.1/24.1/26.7 ms
    if (nchunks == 1) {
        if (int rc = upload(h, {{h->d_stage1, h_imgs1, img * B}, {h->d_stage2, h_imgs2, img * B}})) return rc;
        return rpe_estimate_batch_device(h, h->d_stage1, h->d_stage2, B, K, R, t, inliers, n_matches, status);
    }
    if (!h->copy_stream) {
        HIPCHK(h, hipStreamCreate(&h->copy_stream));
        for (int c = 0; c < 8; ++c) HIPCHK(h, hipEventCreateWithFlags(&h->ev_up[c], hipEventDisableTiming));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));                 // the staging buffers are free again
    const int per = (B + nchunks - 1) / nchunks;
    auto upload_chunk = [&](int c) -> int {
        const int off = c * per, n = B - off < per ? B - off : per;
        if (n <= 0) return RPE_OK;
        HIPCHK(h, hipMemcpyAsync(h->d_stage1 + (size_t)off * img, h_imgs1 + (size_t)off * img, img * n, hipMemcpyHostToDevice, h->copy_stream));
        HIPCHK(h, hipMemcpyAsync(h->d_stage2 + (size_t)off * img, h_imgs2 + (size_t)off * img, img * n, hipMemcpyHostToDevice, h->copy_stream));
        HIPCHK(h, hipEventRecord(h->ev_up[c], h->copy_stream));
        return RPE_OK;
    };
    // The chunks run back to back on the compute stream without a host round trip in between: chunk c's results (and capacity
    // flags) are copied device-to-device into a whole-batch block right behind its kernels, the next upload is issued while
    // they run, and the host waits ONCE, at the end (a fetch per chunk cost four stream drains per batch).  Copies from
    // pageable host memory still block the calling thread while they are staged -- after the kernels of the chunk before
    // have been queued; page-locked batches (rpe_host_alloc / rpe_host_register) do not block at all.
    const size_t MB = (size_t)h->cfg.max_batch;
    const ResultBlock rb(h);
    DM_ONCE(h, h->d_resall, rb.bytes);
    DM_ONCE(h, h->d_ovfall, MB * 2);
    int rc = upload_chunk(0);
    if (rc) return rc;
    for (int c = 0; c < nchunks; ++c) {
        const int off = c * per, n = B - off < per ? B - off : per;
        if (n <= 0) break;
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_up[c], 0));
        if ((rc = rpe_enqueue_batch_device(h, h->d_stage1 + (size_t)off * img, h->d_stage2 + (size_t)off * img, n, K)) != RPE_OK) return rc;
        for (int k = 0; k < RPE_RESULT_SECTIONS; ++k)
            HIPCHK(h, hipMemcpyAsync(h->d_resall + rb.off[k] + (size_t)off * kRpeResultElem[k], h->d_resblk + rb.off[k], (size_t)n * kRpeResultElem[k], hipMemcpyDeviceToDevice, h->stream));
        // the chunk's capacity flags (image slots p and n + p of this launch), before the next chunk overwrites them
        HIPCHK(h, hipMemcpyAsync(h->d_ovfall + off, h->d_ovf, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_ovfall + MB + off, h->d_ovf + n, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToDevice, h->stream));
        if (c + 1 < nchunks && (rc = upload_chunk(c + 1)) != RPE_OK) return rc;
    }
    std::vector<unsigned> ov(2 * MB);
    HIPCHK(h, hipMemcpyAsync(h->h_resblk, h->d_resall, rb.bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(ov.data(), h->d_ovfall, sizeof(unsigned) * 2 * MB, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    unpack_results(h, B, R, t, inliers, n_matches, status);
    last_run_begin(h, RpeLastRun::CHUNKED, rpe_run_batch(h, B), nullptr, nullptr, ov.data());
    return RPE_OK;
}

extern "C" int rpe_fetch_matched_points(rpe_handle *h, int B, float *pts1, float *pts2)
{
    if (!h || B < 1 || B > h->cfg.max_batch) return rpe_invalid(h, "rpe_fetch_matched_points");
    int rc = last_run_gate(h, "rpe_fetch_matched_points", B, NEED_UNCHUNKED);
    if (rc) return rc;
    const size_t n = sizeof(float2) * (size_t)B * h->cfg.max_matches;
    return fetch(h, {{pts1, h->d_pts1, n}, {pts2, h->d_pts2, n}});
}

extern "C" int rpe_fetch_structure(rpe_handle *h, int B, uint8_t *ransac_mask, uint8_t *pose_mask, double *points)
{
    if (!h || B < 1 || B > h->cfg.max_batch) return rpe_invalid(h, "rpe_fetch_structure");
    int rc = last_run_gate(h, "rpe_fetch_structure", B, NEED_UNCHUNKED | NEED_PER_MATCH | NEED_COUNT);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = last_run_structure(h, B, true)) != RPE_OK) return rc;
    const size_t n = (size_t)B * h->cfg.max_matches;
    return fetch(h, {{ransac_mask, h->d_mask, n}, {pose_mask, h->d_pose_mask, n}, {points, h->d_points, n * 3 * sizeof(double)}});
}

extern "C" int rpe_fetch_match_indices(rpe_handle *h, int B, int32_t *qidx, int32_t *tidx)
{
    if (!h || B < 1 || B > h->cfg.max_batch) return rpe_invalid(h, "rpe_fetch_match_indices");
    int rc = last_run_gate(h, "rpe_fetch_match_indices", B, NEED_UNCHUNKED);
    if (rc) return rc;
    const size_t mm = (size_t)h->cfg.max_matches, n = sizeof(int) * (size_t)B * mm;
    std::vector<int> cnt((size_t)B);
    if ((rc = fetch(h, {{cnt.data(), h->d_m_n, sizeof(int) * (size_t)B}, {qidx, h->d_m_q, n}, {tidx, h->d_m_t, n}})) != RPE_OK) return rc;
    for (int p = 0; p < B; ++p)
        for (size_t i = (size_t)std::min(std::max(cnt[(size_t)p], 0), (int)mm); i < mm; ++i) {
            if (qidx) qidx[(size_t)p * mm + i] = -1;
            if (tidx) tidx[(size_t)p * mm + i] = -1;
        }
    return RPE_OK;
}

// ---------------------------------------------------------------- frame store
// rpe_frames_* / rpe_enqueue_pairs (NOT in the reference): extraction separated from pairing.  A put extracts n frames in
// the workspace slots [0, n) exactly as a stream does and one scatter kernel moves what the matchers and the status test
// read -- count, flags, kp_pt, descriptors, and the L2 matcher's norm words -- to the frames' store slots.  A pair list
// then launches the batch's own matcher / RANSAC / pose kernels with a (slot1, slot2) table in place of the
// (pair, img2_base + pair) rule.

// Workgroup (x, i): image i of the workspace -> store slot slots[i]; only the image's `count` rows move, 16 bytes per lane
// (the descriptor rows are 32 or 128 bytes; kp_pt and the norm words are 8-byte records: pairs of them when kcap is even,
// which keeps every slot 16-byte aligned, one by one otherwise).
__global__ __launch_bounds__(256) void frames_scatter_kernel(const uint8_t *__restrict__ desc, const float2 *__restrict__ kp_pt,
                                                              const int2 *__restrict__ norm, const int *__restrict__ kp_count,
                                                              const unsigned *__restrict__ ovf, const int *__restrict__ slots,
                                                              int kcap, int desc_bytes, uint8_t *__restrict__ s_desc,
                                                              float2 *__restrict__ s_pt, int2 *__restrict__ s_norm,
                                                              int *__restrict__ s_count, unsigned *__restrict__ s_ovf)
{
    const int img = blockIdx.y, slot = slots[img];
    const int cnt = kp_count[img], n = min(cnt, kcap);
    const int t0 = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
    if (t0 == 0) { s_count[slot] = cnt; s_ovf[slot] = ovf[img]; }
    const long long src = (long long)img * kcap, dst = (long long)slot * kcap;
    const uint4 *d_in = (const uint4 *)(desc + src * desc_bytes);
    uint4 *d_out = (uint4 *)(s_desc + dst * desc_bytes);
    const int nd = n * (desc_bytes >> 4);
    for (int i = t0; i < nd; i += step) d_out[i] = d_in[i];
    if ((kcap & 1) == 0) {
        const int n2 = n >> 1;
        const uint4 *p_in = (const uint4 *)(kp_pt + src); uint4 *p_out = (uint4 *)(s_pt + dst);
        for (int i = t0; i < n2; i += step) p_out[i] = p_in[i];
        if ((n & 1) && t0 == 0) s_pt[dst + n - 1] = kp_pt[src + n - 1];
        if (norm) {
            const uint4 *n_in = (const uint4 *)(norm + src); uint4 *n_out = (uint4 *)(s_norm + dst);
            for (int i = t0; i < n2; i += step) n_out[i] = n_in[i];
            if ((n & 1) && t0 == 0) s_norm[dst + n - 1] = norm[src + n - 1];
        }
    } else {
        for (int i = t0; i < n; i += step) s_pt[dst + i] = kp_pt[src + i];
        if (norm) for (int i = t0; i < n; i += step) s_norm[dst + i] = norm[src + i];
    }
}

// the norm words are read by the matrix-core L2 kernels: the crossCheck matcher, and the guided matcher of either match
// mode (the Lowe-ratio matcher itself runs on the vector ALU and computes its own).  Every NORM_L2 handle keeps them, so
// a pair list of any L2 handle can be matched again under a pose
static bool frames_keep_norms(const rpe_handle *h) { return h->cfg.norm_type == RPE_NORM_L2; }

extern "C" int rpe_frames_capacity(const rpe_handle *h) { return h ? h->fs.cap : 0; }

extern "C" int rpe_frames_reserve(rpe_handle *h, int n_slots)
{
    if (!h) return rpe_invalid(h, "rpe_frames_reserve");
    if (n_slots < 0 || n_slots > (1 << 24)) { h->err = "rpe_frames_reserve: n_slots must be 0 ... 16777216"; return RPE_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (n_slots == h->fs.cap) return RPE_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));            // nothing in flight reads the store that is about to go
    last_run_store_changed(h, true);
    if (n_slots == 0) { frames_free(h->fs); return RPE_OK; }
    const size_t kcap = (size_t)h->lay.kcap, db = (size_t)h->desc_bytes, N = (size_t)n_slots;
    const bool l2 = frames_keep_norms(h);
    rpe_handle::FrameStore nf;
    bool ok = hipMalloc((void **)&nf.d_desc, N * kcap * db) == hipSuccess && hipMalloc((void **)&nf.d_kp_pt, N * kcap * sizeof(float2)) == hipSuccess &&
              (!l2 || hipMalloc((void **)&nf.d_norm, N * kcap * sizeof(int2)) == hipSuccess) &&
              hipMalloc((void **)&nf.d_count, N * sizeof(int)) == hipSuccess && hipMalloc((void **)&nf.d_ovf, N * sizeof(unsigned)) == hipSuccess &&
              hipMalloc((void **)&nf.d_cam, N * sizeof(rpe_camera)) == hipSuccess;
    const size_t keep = (size_t)(h->fs.cap < n_slots ? h->fs.cap : n_slots);
    ok = ok && hipMemsetAsync(nf.d_count, 0, N * sizeof(int), h->stream) == hipSuccess && hipMemsetAsync(nf.d_ovf, 0, N * sizeof(unsigned), h->stream) == hipSuccess &&
         hipMemsetAsync(nf.d_cam, 0, N * sizeof(rpe_camera), h->stream) == hipSuccess;
    if (ok && keep) {
        ok = hipMemcpyAsync(nf.d_desc, h->fs.d_desc, keep * kcap * db, hipMemcpyDeviceToDevice, h->stream) == hipSuccess &&
             hipMemcpyAsync(nf.d_kp_pt, h->fs.d_kp_pt, keep * kcap * sizeof(float2), hipMemcpyDeviceToDevice, h->stream) == hipSuccess &&
             (!l2 || hipMemcpyAsync(nf.d_norm, h->fs.d_norm, keep * kcap * sizeof(int2), hipMemcpyDeviceToDevice, h->stream) == hipSuccess) &&
             hipMemcpyAsync(nf.d_count, h->fs.d_count, keep * sizeof(int), hipMemcpyDeviceToDevice, h->stream) == hipSuccess &&
             hipMemcpyAsync(nf.d_ovf, h->fs.d_ovf, keep * sizeof(unsigned), hipMemcpyDeviceToDevice, h->stream) == hipSuccess &&
             hipMemcpyAsync(nf.d_cam, h->fs.d_cam, keep * sizeof(rpe_camera), hipMemcpyDeviceToDevice, h->stream) == hipSuccess;
    }
    ok = ok && hipStreamSynchronize(h->stream) == hipSuccess;
    if (!ok) {
        const hipError_t e = hipGetLastError();
        char b[256];
        snprintf(b, sizeof(b), "rpe_frames_reserve: could not build a store of %d slots (%s); the old store of %d slots is kept", n_slots, hipGetErrorString(e), h->fs.cap);
        frames_free(nf);
        h->err = b;
        return RPE_ERR_HIP;
    }
    nf.cap = n_slots;
    nf.filled.assign(N, 0);
    nf.has_cam.assign(N, 0);
    nf.h_cam.assign(N, rpe_camera{});
    for (size_t i = 0; i < keep; ++i) { nf.filled[i] = h->fs.filled[i]; nf.has_cam[i] = h->fs.has_cam[i]; nf.h_cam[i] = h->fs.h_cam[i]; }
    rpe_handle::FrameStore old = h->fs;
    h->fs = nf;
    frames_free(old);
    return RPE_OK;
}

// The caller's slot arrays go through a ring of pinned buffers (the caller may reuse its arrays as soon as the call
// returns, and the host may run RPE_TAB_RING calls ahead of the stream) and from there to d_pairtab on the handle's stream
static int upload_table(rpe_handle *h, const int32_t *a, const int32_t *b, int n)
{
    const size_t per = (size_t)2 * h->cfg.max_batch;                 // ints: 2*max_batch put slots or max_batch (slot1, slot2) entries
    if (!h->h_pairtab) {
        HIPCHK(h, hipHostMalloc((void **)&h->h_pairtab, RPE_TAB_RING * per * sizeof(int)));
        DM(h, h->d_pairtab, per);
        for (int i = 0; i < RPE_TAB_RING; ++i) HIPCHK(h, hipEventCreateWithFlags(&h->ev_tab[i], hipEventDisableTiming));
    }
    const int r = h->tab_next;
    h->tab_next = (r + 1) % RPE_TAB_RING;
    HIPCHK(h, hipEventSynchronize(h->ev_tab[r]));                     // the upload that last used this piece has run
    int *dst = h->h_pairtab + (size_t)r * per;
    if (b) for (int i = 0; i < n; ++i) { dst[2 * i] = a[i]; dst[2 * i + 1] = b[i]; }
    else memcpy(dst, a, sizeof(int) * (size_t)n);
    if (int rc = upload(h, {{h->d_pairtab, dst, sizeof(int) * (size_t)(b ? 2 * n : n)}})) return rc;
    HIPCHK(h, hipEventRecord(h->ev_tab[r], h->stream));
    return RPE_OK;
}

static int frames_check_put(rpe_handle *h, const void *frames, int n, const int32_t *slots)
{
    if (!h || !frames || !slots || n < 1) { if (h) h->err = "rpe_frames_put: null argument or n < 1"; return RPE_ERR_INVALID; }
    if (n > h->n_img_cap) { h->err = "rpe_frames_put: more than 2*max_batch frames in one call"; return RPE_ERR_CAPACITY; }
    if (h->fs.cap == 0) { h->err = "rpe_frames_put: no frame store (rpe_frames_reserve)"; return RPE_ERR_INVALID; }
    std::vector<int32_t> s(slots, slots + n);
    std::sort(s.begin(), s.end());
    if (s.front() < 0 || s.back() >= h->fs.cap) { h->err = "rpe_frames_put: slot outside the store"; return RPE_ERR_INVALID; }
    for (int i = 1; i < n; ++i) if (s[i] == s[i - 1]) { h->err = "rpe_frames_put: a slot appears twice in one put"; return RPE_ERR_INVALID; }
    return RPE_OK;
}

// extraction of na + nb images (workspace slots [0, na + nb), as a stream / the stage API place them) + scatter
static int frames_put_run(rpe_handle *h, const uint8_t *d_a, const uint8_t *d_b, int na, int nb, const int32_t *slots)
{
    const int n = na + nb;
    int rc = upload_table(h, slots, nullptr, n);
    if (rc) return rc;
    last_run_end(h, true);      // the workspace's per-image arrays are overwritten: what described "the last batch" through them is gone
    h->ev_valid = false;
    if (h->cfg.feature_method == RPE_FEATURE_SIFT) rc = rpe_sift_run(h, d_a, d_b, na, nb);
    else rc = run_orb(h, d_a, d_b, na, nb);
    if (rc) return rc;
    const bool l2 = frames_keep_norms(h);
    if (l2) rpe_launch_l2_norms(h, n);
    const int rows = h->lay.kcap * (h->desc_bytes >> 4);               // 16-byte pieces of a full image's descriptors
    const int gx = rows >= 65536 ? 32 : rows >= 8192 ? 8 : 2;
    hipLaunchKernelGGL(frames_scatter_kernel, dim3(gx, n), dim3(256), 0, h->stream,
                       (const uint8_t *)h->d_desc, (const float2 *)h->d_kp_pt, l2 ? (const int2 *)h->d_m_norm : (const int2 *)nullptr,
                       (const int *)h->d_kp_count, (const unsigned *)h->d_ovf, (const int *)h->d_pairtab, h->lay.kcap, h->desc_bytes,
                       h->fs.d_desc, h->fs.d_kp_pt, h->fs.d_norm, h->fs.d_count, h->fs.d_ovf);
    HIPCHK(h, hipGetLastError());
    for (int i = 0; i < n; ++i) h->fs.filled[(size_t)slots[i]] = 1;
    return RPE_OK;
}

extern "C" int rpe_frames_put_device(rpe_handle *h, const uint8_t *d_frames, int n, const int32_t *slots)
{
    int rc = frames_check_put(h, d_frames, n, slots);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return frames_put_run(h, d_frames, d_frames, n, 0, slots);
}

extern "C" int rpe_frames_put(rpe_handle *h, const uint8_t *h_frames, int n, const int32_t *slots)
{
    int rc = frames_check_put(h, h_frames, n, slots);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int na, nb;
    if ((rc = stage_images(h, h_frames, n, na, nb)) != RPE_OK) return rc;
    return frames_put_run(h, h->d_stage1, h->d_stage2, na, nb, slots);
}

extern "C" int rpe_frames_info(rpe_handle *h, int n, const int32_t *slots, int32_t *counts, uint32_t *flags)
{
    if (!h || !slots || n < 1) { if (h) h->err = "rpe_frames_info: null argument or n < 1"; return RPE_ERR_INVALID; }
    if (h->fs.cap == 0) { h->err = "rpe_frames_info: no frame store (rpe_frames_reserve)"; return RPE_ERR_INVALID; }
    for (int i = 0; i < n; ++i) if (slots[i] < 0 || slots[i] >= h->fs.cap) { h->err = "rpe_frames_info: slot outside the store"; return RPE_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int lo = slots[0], hi = slots[0];
    for (int i = 1; i < n; ++i) { lo = std::min(lo, (int)slots[i]); hi = std::max(hi, (int)slots[i]); }
    const size_t span = (size_t)(hi - lo + 1);                 // the range the call names, not the whole store
    std::vector<int> cnt(span);
    std::vector<unsigned> ov(span);
    if (int rc = fetch(h, {{cnt.data(), h->fs.d_count + lo, sizeof(int) * span}, {ov.data(), h->fs.d_ovf + lo, sizeof(unsigned) * span}})) return rc;
    for (int i = 0; i < n; ++i) {
        const size_t s = (size_t)slots[i];
        const bool f = h->fs.filled[s] != 0;
        if (counts) counts[i] = f ? cnt[s - lo] : -1;
        if (flags) flags[i] = f ? ov[s - lo] : 0u;
    }
    return RPE_OK;
}

// K == nullptr: the camera form, every pair on the cameras of its two slots
static int enqueue_pairs_run(rpe_handle *h, const int32_t *slot1, const int32_t *slot2, int P, const double *K, const char *who)
{
    const char *bad = nullptr;
    int rc = RPE_ERR_INVALID;
    if (P > h->cfg.max_batch) { bad = ": pair list exceeds max_batch"; rc = RPE_ERR_CAPACITY; }
    else if (h->fs.cap == 0) bad = ": no frame store (rpe_frames_reserve)";
    for (int p = 0; p < P && !bad; ++p) {
        if (slot1[p] < 0 || slot1[p] >= h->fs.cap || slot2[p] < 0 || slot2[p] >= h->fs.cap) bad = ": slot outside the store";
        else if (!h->fs.filled[(size_t)slot1[p]] || !h->fs.filled[(size_t)slot2[p]]) bad = ": a pair names an empty slot";
        else if (!K && (!h->fs.has_cam[(size_t)slot1[p]] || !h->fs.has_cam[(size_t)slot2[p]])) bad = ": a pair names a slot without a camera (rpe_frames_set_cameras)";
    }
    if (bad) { h->err = std::string(who) + bad; return rc; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (K && (rc = set_K(h, K)) != RPE_OK) return rc;
    if ((rc = upload_table(h, slot1, slot2, P)) != RPE_OK) return rc;
    const RpeRun r = rpe_run_list(h, P, K ? RpeCamSrc{nullptr, nullptr, 0} : RpeCamSrc{h->fs.d_cam, (const int2 *)h->d_pairtab, 0});
    last_run_begin(h, RpeLastRun::LIST, r, slot1, slot2);
    MARK(h, RPE_STAGE_MATCH);
    if ((rc = run_tail(h, r)) != RPE_OK) last_run_end(h);
    return rc;
}

extern "C" int rpe_enqueue_pairs(rpe_handle *h, const int32_t *slot1, const int32_t *slot2, int P, const double K[9])
{
    if (!h || !slot1 || !slot2 || !K || P < 1) { if (h) h->err = "rpe_enqueue_pairs: null argument or P < 1"; return RPE_ERR_INVALID; }
    return enqueue_pairs_run(h, slot1, slot2, P, K, "rpe_enqueue_pairs");
}

extern "C" int rpe_estimate_pairs(rpe_handle *h, const int32_t *slot1, const int32_t *slot2, int P, const double K[9],
                                  double *R, double *t, int32_t *inliers, int32_t *n_matches, int32_t *status)
{
    int rc = rpe_enqueue_pairs(h, slot1, slot2, P, K);
    if (rc) return rc;
    return rpe_fetch_results(h, P, R, t, inliers, n_matches, status);
}

// ---------------------------------------------------------------- stage API
extern "C" int rpe_orb_detect_and_compute(rpe_handle *h, const uint8_t *h_imgs, int n_images,
                                          rpe_keypoint *kps, uint8_t *desc, int32_t *counts)
{
    if (!h || !h_imgs || n_images < 1) return rpe_invalid(h, "rpe_orb_detect_and_compute");
    if (h->cfg.feature_method != RPE_FEATURE_ORB) { h->err = "handle was not created for ORB"; return RPE_ERR_INVALID; }
    if (n_images > h->n_img_cap) { h->err = "n_images exceeds 2*max_batch"; return RPE_ERR_CAPACITY; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    last_run_end(h);                            // overwrites buffers rpe_fetch_structure reads
    int na, nb;
    int rc = stage_images(h, h_imgs, n_images, na, nb);
    if (rc == RPE_OK) rc = run_orb(h, h->d_stage1, h->d_stage2, na, nb);
    if (rc) return rc;
    const int kcap = h->lay.kcap;
    std::vector<unsigned> xy((size_t)n_images * kcap);
    std::vector<float> resp((size_t)n_images * kcap), ang((size_t)n_images * kcap);
    std::vector<float2> pt((size_t)n_images * kcap);
    std::vector<int> cnt(n_images);
    rc = fetch(h, {{xy.data(), h->d_kp_xy, xy.size() * 4}, {resp.data(), h->d_kp_resp, resp.size() * 4}, {ang.data(), h->d_kp_angle, ang.size() * 4},
                   {pt.data(), h->d_kp_pt, pt.size() * 8}, {cnt.data(), h->d_kp_count, cnt.size() * 4}, {desc, h->d_desc, (size_t)n_images * kcap * 32}});
    if (rc) return rc;
    for (int i = 0; i < n_images; ++i) {
        if (counts) counts[i] = cnt[i];
        if (!kps) continue;
        for (int k = 0; k < cnt[i]; ++k) {
            size_t g = (size_t)i * kcap + k;
            rpe_keypoint &o = kps[g];
            o.x = pt[g].x; o.y = pt[g].y; o.angle = ang[g]; o.response = resp[g];
            o.octave = (int)(xy[g] >> 24); o.lx = (int)(xy[g] & 0xFFF); o.ly = (int)((xy[g] >> 12) & 0xFFF);
        }
    }
    return RPE_OK;
}

extern "C" int64_t rpe_orb_pyramid_pixels(const rpe_handle *h)
{
    if (!h) return 0;
    int64_t n = 0;
    for (int l = 0; l < RPE_NLEVELS; ++l) n += (int64_t)h->lay.lv[l].w * h->lay.lv[l].h;
    return n;
}

extern "C" int rpe_orb_group_min_images(void) { return RPE_ORB_GROUP_MIN_IMAGES; }

extern "C" int rpe_orb_debug_fetch(rpe_handle *h, int index, int which, uint8_t *h_out)
{
    if (!h || !h_out || index < 0 || index >= h->n_img_cap) return rpe_invalid(h, "rpe_orb_debug_fetch");
    if (h->cfg.feature_method != RPE_FEATURE_ORB) { h->err = "rpe_orb_debug_fetch: handle was not created for ORB"; return RPE_ERR_INVALID; }
    if (which != 0 && which != 2 && which != 3) { h->err = "rpe_orb_debug_fetch: which must be 0 (pyramid), 2 (NMS map) or 3 (blurred pyramid)"; return RPE_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    std::vector<uint8_t> tmp((size_t)h->lay.stride, 0);
    if (which == 2) {
        // the NMS map is not materialised any more: rebuild it from the tile lists of the image
        const size_t nt = (size_t)h->n_tiles_fast;
        std::vector<int> cnt(nt ? nt : 1);
        std::vector<unsigned> lst((nt ? nt : 1) * RPE_FAST_TILE_CAP);
        if (nt) {
            HIPCHK(h, hipMemcpyAsync(cnt.data(), h->d_tile_cnt + (size_t)index * nt, nt * sizeof(int), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipMemcpyAsync(lst.data(), h->d_tile_list + (size_t)index * nt * RPE_FAST_TILE_CAP, nt * RPE_FAST_TILE_CAP * sizeof(unsigned),
                                     hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        for (int l = 0; l < RPE_NLEVELS; ++l) {
            const RpeLevel &v = h->lay.lv[l];
            for (int t = v.tile0; t < v.tile0 + v.ntile; ++t)
                for (int k = 0; k < cnt[t] && k < RPE_FAST_TILE_CAP; ++k) {
                    const unsigned e = lst[(size_t)t * RPE_FAST_TILE_CAP + k];
                    tmp[v.off + (size_t)((e >> 12) & 0xFFF) * v.pitch + (e & 0xFFF)] = (uint8_t)(e >> 24);
                }
        }
    } else {
        const uint8_t *src = h->d_pyr + (size_t)index * h->lay.stride;
        if (h->lay.in_a) {
            // level 0 of the last run was read in place: bring this image's copy into the pyramid-shaped buffer (the
            // batches handed to the last enqueue must still be alive, as they are for the host-buffer entry points)
            if (index >= h->level0_slots) { h->err = "rpe_orb_debug_fetch: image slot was not part of the last run"; return RPE_ERR_INVALID; }
            const size_t img = (size_t)h->lay.in_img;
            const uint8_t *in = index < h->lay.in_na ? h->lay.in_a + (size_t)index * img : h->lay.in_b + (size_t)(index - h->lay.in_na) * img;
            HIPCHK(h, hipMemcpyAsync(h->d_pyr + (size_t)index * h->lay.stride + h->lay.lv[0].off, in, img, hipMemcpyDeviceToDevice, h->stream));
        }
        if (which == 3) { rpe_launch_debug_blur(h, index); HIPCHK(h, hipGetLastError()); src = h->d_bufA; }
        HIPCHK(h, hipMemcpyAsync(tmp.data(), src, tmp.size(), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    uint8_t *o = h_out;
    for (int l = 0; l < RPE_NLEVELS; ++l) {
        const RpeLevel &v = h->lay.lv[l];
        for (int y = 0; y < v.h; ++y, o += v.w) memcpy(o, tmp.data() + v.off + (size_t)y * v.pitch, v.w);
    }
    return RPE_OK;
}

extern "C" int rpe_orb_debug_retain(rpe_handle *h, int kind, int stl_runtime, void *elems, const int32_t *len, const int32_t *n_points,
                                    int n_lists, int cap, int32_t *out_len)
{
    if (!h || !elems || !len || !n_points || !out_len || n_lists < 1 || cap < 1) return rpe_invalid(h, "rpe_orb_debug_retain");
    if (h->cfg.feature_method != RPE_FEATURE_ORB) return rpe_invalid(h, "rpe_orb_debug_retain", "handle was not created for ORB");
    if (kind != 0 && kind != 1) return rpe_invalid(h, "rpe_orb_debug_retain", "kind must be 0 (u32 FAST entries) or 1 (u64 Harris entries)");
    if (stl_runtime != RPE_STL_LIBSTDCXX && stl_runtime != RPE_STL_MSVC) return rpe_invalid(h, "rpe_orb_debug_retain", "unknown stl_runtime");
    // positions travel as u16 and the list, with its stopper positions, must fit the default dynamic LDS of a workgroup
    if (cap > 8192 || rpe_retain_lds(kind, cap) > RPE_LDS_DEFAULT_BYTES) return rpe_invalid(h, "rpe_orb_debug_retain", "cap too large for one workgroup's LDS");
    for (int i = 0; i < n_lists; ++i)
        if (len[i] < 0 || len[i] > cap) return rpe_invalid(h, "rpe_orb_debug_retain", "a list is longer than the capacity the launch is sized for");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t esz = kind ? 8 : 4, bytes = esz * (size_t)n_lists * cap, ibytes = sizeof(int) * (size_t)n_lists;
    void *d_elems = nullptr; int *d_int = nullptr;                   // len | n_points | out_len
    HIPCHK(h, hipMalloc(&d_elems, bytes));
    hipError_t e = hipMalloc((void **)&d_int, 3 * ibytes);
    if (e == hipSuccess) e = hipMemcpyAsync(d_elems, elems, bytes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_int, len, ibytes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_int + n_lists, n_points, ibytes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) {
        rpe_launch_debug_retain(h, kind, stl_runtime, d_elems, d_int, d_int + n_lists, d_int + 2 * (size_t)n_lists, n_lists, cap);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(elems, d_elems, bytes, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out_len, d_int + 2 * (size_t)n_lists, ibytes, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    hipFree(d_elems); hipFree(d_int);
    HIPCHK(h, e);
    return RPE_OK;
}

// tail of rpe_match_hamming / rpe_match_l2 (descriptors of pair p uploaded to workspace slots p and B + p): counts,
// the handle's matcher of that norm, the match lists (dist: int32 Hamming distances or f32 L2 distances, 4 bytes either)
static int stage_match_run(rpe_handle *h, bool l2, const int32_t *n1, const int32_t *n2, int B, int32_t *qidx, int32_t *tidx,
                           void *dist, int32_t *n_matches)
{
    const size_t mm = h->cfg.max_matches;
    if (int rc = upload_counts(h, n1, n2, B)) return rc;
    if (l2) rpe_launch_match_l2(h, rpe_run_batch(h, B));
    else rpe_launch_match(h, rpe_run_batch(h, B));
    HIPCHK(h, hipGetLastError());
    return fetch(h, {{qidx, h->d_m_q, sizeof(int) * mm * B}, {tidx, h->d_m_t, sizeof(int) * mm * B}, {dist, h->d_m_d, sizeof(int) * mm * B},
                     {n_matches, h->d_m_n, sizeof(int) * B}});
}

extern "C" int rpe_match_hamming(rpe_handle *h, const uint8_t *h_desc1, const int32_t *n1, const uint8_t *h_desc2,
                                 const int32_t *n2, int B, int32_t *qidx, int32_t *tidx, int32_t *dist, int32_t *n_matches)
{
    if (!h || !h_desc1 || !h_desc2 || !n1 || !n2 || B < 1) return rpe_invalid(h, "rpe_match_hamming");
    if (int rc = check_batch(h, B)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    last_run_end(h);                            // overwrites buffers rpe_fetch_structure reads
    if (int rc = check_desc_counts(h, n1, B)) return rc;
    if (int rc = check_desc_counts(h, n2, B)) return rc;
    if (int rc = upload_descriptors(h, h_desc1, h_desc2, B)) return rc;
    return stage_match_run(h, false, n1, n2, B, qidx, tidx, dist, n_matches);
}

static int upload_points(rpe_handle *h, const float *p1, const float *p2, const int32_t *m, int B)
{
    const size_t mm = h->cfg.max_matches;
    if (int rc = check_match_counts(h, m, B)) return rc;
    return upload(h, {{h->d_pts1, p1, sizeof(float2) * mm * B}, {h->d_pts2, p2, sizeof(float2) * mm * B}, {h->d_m_n, m, sizeof(int) * B}});
}

// ---------------------------------------------------------------- camera models
// rpe_*_cameras (NOT in the reference): a camera per frame instead of one K per call.  The entry points validate, place
// the camera records where the kernels find them -- 2 B records per batch / stage call in d_batch_cams, one record per
// frame-store slot in fs.d_cam -- and name them in the camera source of the run they launch, which makes the launchers of
// geom_kernels.hip and link_kernels.hip take the camera instances (launch_cam, geom_device.h).
int check_cameras(rpe_handle *h, const rpe_camera *c, int n, const char *who)
{
    for (int i = 0; i < n; ++i) {
        const double *f = &c[i].fx;                     // fx fy cx cy dist[8]: twelve doubles
        bool fin = true;
        for (int k = 0; k < 12; ++k) fin = fin && std::isfinite(f[k]);
        if (!fin) { h->err = std::string(who) + ": a camera has a non-finite field"; return RPE_ERR_INVALID; }
        if (!(c[i].fx > 0.) || !(c[i].fy > 0.)) { h->err = std::string(who) + ": a camera has fx <= 0 or fy <= 0"; return RPE_ERR_INVALID; }
    }
    return RPE_OK;
}

// cam1[0, B) then cam2[0, B): the image-slot order of a batch (pair p = records p and B + p)
static int upload_batch_cameras(rpe_handle *h, const rpe_camera *cam1, const rpe_camera *cam2, int B)
{
    const size_t cap = (size_t)2 * h->cfg.max_batch;
    if (!h->d_batch_cams) {
        DM(h, h->d_batch_cams, cap);
        h->h_batch_cams.resize(cap);
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));      // nothing in flight reads the records or their staging
    memcpy(h->h_batch_cams.data(), cam1, sizeof(rpe_camera) * (size_t)B);
    memcpy(h->h_batch_cams.data() + B, cam2, sizeof(rpe_camera) * (size_t)B);
    return upload(h, {{h->d_batch_cams, h->h_batch_cams.data(), sizeof(rpe_camera) * 2 * (size_t)B}});
}

extern "C" int rpe_frames_set_cameras(rpe_handle *h, int n, const int32_t *slots, const rpe_camera *cams)
{
    if (!h || !slots || !cams || n < 1) { if (h) h->err = "rpe_frames_set_cameras: null argument or n < 1"; return RPE_ERR_INVALID; }
    if (h->fs.cap == 0) { h->err = "rpe_frames_set_cameras: no frame store (rpe_frames_reserve)"; return RPE_ERR_INVALID; }
    for (int i = 0; i < n; ++i) if (slots[i] < 0 || slots[i] >= h->fs.cap) { h->err = "rpe_frames_set_cameras: slot outside the store"; return RPE_ERR_INVALID; }
    int rc = check_cameras(h, cams, n, "rpe_frames_set_cameras");
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));      // a pair list in flight may read the records about to change
    last_run_store_changed(h, false);
    for (int i = 0; i < n; ++i) {
        const size_t s = (size_t)slots[i];
        h->fs.h_cam[s] = cams[i];
        h->fs.has_cam[s] = 1;
        if ((rc = upload(h, {{h->fs.d_cam + s, &h->fs.h_cam[s], sizeof(rpe_camera)}})) != RPE_OK) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return RPE_OK;
}

extern "C" int rpe_enqueue_pairs_cameras(rpe_handle *h, const int32_t *slot1, const int32_t *slot2, int P)
{
    if (!h || !slot1 || !slot2 || P < 1) { if (h) h->err = "rpe_enqueue_pairs_cameras: null argument or P < 1"; return RPE_ERR_INVALID; }
    return enqueue_pairs_run(h, slot1, slot2, P, nullptr, "rpe_enqueue_pairs_cameras");
}

extern "C" int rpe_estimate_pairs_cameras(rpe_handle *h, const int32_t *slot1, const int32_t *slot2, int P,
                                          double *R, double *t, int32_t *inliers, int32_t *n_matches, int32_t *status)
{
    int rc = rpe_enqueue_pairs_cameras(h, slot1, slot2, P);
    if (rc) return rc;
    return rpe_fetch_results(h, P, R, t, inliers, n_matches, status);
}

extern "C" int rpe_enqueue_batch_cameras_device(rpe_handle *h, const uint8_t *d_imgs1, const uint8_t *d_imgs2, int B,
                                                const rpe_camera *cam1, const rpe_camera *cam2)
{
    if (!h || !d_imgs1 || !d_imgs2 || !cam1 || !cam2 || B < 1) { if (h) h->err = "rpe_enqueue_batch_cameras_device: null argument or B < 1"; return RPE_ERR_INVALID; }
    if (int rc = check_batch(h, B)) return rc;
    int rc = check_cameras(h, cam1, B, "rpe_enqueue_batch_cameras_device");
    if (!rc) rc = check_cameras(h, cam2, B, "rpe_enqueue_batch_cameras_device");
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = upload_batch_cameras(h, cam1, cam2, B)) != RPE_OK) return rc;
    // plain launches whatever B: the captured graphs hold the shared-K instances
    return run_images(h, d_imgs1, d_imgs2, B, B, rpe_run_batch(h, B, RpeCamSrc{h->d_batch_cams, nullptr, B}));
}

extern "C" int rpe_estimate_batch_cameras_device(rpe_handle *h, const uint8_t *d_imgs1, const uint8_t *d_imgs2, int B,
                                                 const rpe_camera *cam1, const rpe_camera *cam2, double *R, double *t,
                                                 int32_t *inliers, int32_t *n_matches, int32_t *status)
{
    int rc = rpe_enqueue_batch_cameras_device(h, d_imgs1, d_imgs2, B, cam1, cam2);
    if (rc) return rc;
    return rpe_fetch_results(h, B, R, t, inliers, n_matches, status);
}

extern "C" int rpe_estimate_batch_cameras(rpe_handle *h, const uint8_t *h_imgs1, const uint8_t *h_imgs2, int B,
                                          const rpe_camera *cam1, const rpe_camera *cam2, double *R, double *t,
                                          int32_t *inliers, int32_t *n_matches, int32_t *status)
{
    if (!h || !h_imgs1 || !h_imgs2 || !cam1 || !cam2 || B < 1) { if (h) h->err = "rpe_estimate_batch_cameras: null argument or B < 1"; return RPE_ERR_INVALID; }
    if (int rc = check_batch(h, B)) return rc;
    const size_t img = (size_t)h->cfg.width * h->cfg.height;
    if (batch_is_chunked(h, B)) {
        h->err = "rpe_estimate_batch_cameras: host batches this large (B >= 512 and >= 64 MiB per image set) are not chunked by the camera form: upload the images and call rpe_estimate_batch_cameras_device";
        return RPE_ERR_INVALID;
    }
    int rc = check_cameras(h, cam1, B, "rpe_estimate_batch_cameras");
    if (!rc) rc = check_cameras(h, cam2, B, "rpe_estimate_batch_cameras");
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = upload(h, {{h->d_stage1, h_imgs1, img * B}, {h->d_stage2, h_imgs2, img * B}})) != RPE_OK) return rc;
    return rpe_estimate_batch_cameras_device(h, h->d_stage1, h->d_stage2, B, cam1, cam2, R, t, inliers, n_matches, status);
}

extern "C" int rpe_undistort_points(rpe_handle *h, const float *h_pts, int n, const rpe_camera *cam, double *h_out_xy)
{
    if (!h || !h_pts || !cam || !h_out_xy || n < 1) { if (h) h->err = "rpe_undistort_points: null argument or n < 1"; return RPE_ERR_INVALID; }
    int rc = check_cameras(h, cam, 1, "rpe_undistort_points");
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    void *d_in = nullptr, *d_out = nullptr, *d_cam = nullptr;
    const size_t nb_in = sizeof(float2) * (size_t)n, nb_out = sizeof(double2) * (size_t)n;
    bool ok = hipMalloc(&d_in, nb_in) == hipSuccess && hipMalloc(&d_out, nb_out) == hipSuccess && hipMalloc(&d_cam, sizeof(rpe_camera)) == hipSuccess;
    ok = ok && hipMemcpyAsync(d_in, h_pts, nb_in, hipMemcpyHostToDevice, h->stream) == hipSuccess &&
         hipMemcpyAsync(d_cam, cam, sizeof(rpe_camera), hipMemcpyHostToDevice, h->stream) == hipSuccess;
    if (ok) {
        rpe_launch_undistort(h, (const float2 *)d_in, n, (const rpe_camera *)d_cam, (double2 *)d_out);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(h_out_xy, d_out, nb_out, hipMemcpyDeviceToHost, h->stream) == hipSuccess;
    }
    ok = (hipStreamSynchronize(h->stream) == hipSuccess) && ok;
    if (d_in) hipFree(d_in);
    if (d_out) hipFree(d_out);
    if (d_cam) hipFree(d_cam);
    if (!ok) { (void)hipGetLastError(); h->err = "rpe_undistort_points: HIP failure"; return RPE_ERR_HIP; }
    return RPE_OK;
}

// ---------------------------------------------------------------- stage API: geometry
// findEssentialMat, recoverPose and the refinement over uploaded points, each on one K (rpe_*) or on a camera per side and
// pair (rpe_*_cameras, K == nullptr here).  Head of the three: capacity, cameras, points and intrinsics resident; `run`
// is the stage run over the B uploaded pairs.
int stage_begin(rpe_handle *h, const char *who, const float *p1, const float *p2, const int32_t *m, int B,
                       const double *K, const rpe_camera *cam1, const rpe_camera *cam2, RpeRun &run)
{
    if (int rc = check_batch(h, B)) return rc;
    int rc = RPE_OK;
    if (!K && (rc = check_cameras(h, cam1, B, who)) == RPE_OK) rc = check_cameras(h, cam2, B, who);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    last_run_end(h);                            // overwrites buffers rpe_fetch_structure reads
    if (!K && (rc = upload_batch_cameras(h, cam1, cam2, B)) != RPE_OK) return rc;
    if ((rc = upload_points(h, p1, p2, m, B)) != RPE_OK) return rc;
    if (K && (rc = set_K(h, K)) != RPE_OK) return rc;
    run = rpe_run_batch(h, B, K ? RpeCamSrc{nullptr, nullptr, 0} : RpeCamSrc{h->d_batch_cams, nullptr, B});
    return RPE_OK;
}

static int stage_find_essential(rpe_handle *h, const char *who, const float *h_pts1, const float *h_pts2, const int32_t *m, int B,
                                const double *K, const rpe_camera *cam1, const rpe_camera *cam2, double *E, uint8_t *mask,
                                int32_t *found, int32_t *info)
{
    RpeRun run;
    int rc = stage_begin(h, who, h_pts1, h_pts2, m, B, K, cam1, cam2, run);
    if (rc) return rc;
    HIPCHK(h, hipMemsetAsync(h->d_E, 0, sizeof(double) * 9 * B, h->stream));
    rpe_launch_ransac(h, run, true);
    HIPCHK(h, hipGetLastError());
    std::vector<RpeRansacState> st(B);
    if ((rc = fetch(h, {{st.data(), h->d_rstate, sizeof(RpeRansacState) * B}, {mask, h->d_mask, (size_t)h->cfg.max_matches * B}})) != RPE_OK) return rc;
    for (int i = 0; i < B; ++i) {
        if (E) memcpy(E + 9 * i, st[i].E, sizeof(double) * 9);
        if (found) found[i] = st[i].found;
        if (info) { info[4 * i] = st[i].best_count; info[4 * i + 1] = st[i].best_iter; info[4 * i + 2] = st[i].best_model; info[4 * i + 3] = st[i].iters_run; }
    }
    return RPE_OK;
}

static int stage_recover_pose(rpe_handle *h, const char *who, const double *h_E, const float *h_pts1, const float *h_pts2,
                              const int32_t *m, int B, const double *K, const rpe_camera *cam1, const rpe_camera *cam2,
                              double *R, double *t, int32_t *inliers)
{
    RpeRun run;
    int rc = stage_begin(h, who, h_pts1, h_pts2, m, B, K, cam1, cam2, run);
    if (rc) return rc;
    if ((rc = upload(h, {{h->d_E, h_E, sizeof(double) * 9 * B}})) != RPE_OK) return rc;
    if (run.cam.cams) rpe_launch_normalise(h, run);             // recover_pose_kernel's camera instances read d_n1 / d_n2
    rpe_launch_pose(h, run, false);
    HIPCHK(h, hipGetLastError());
    return rpe_fetch_results(h, B, R, t, inliers, nullptr, nullptr);
}

extern "C" int rpe_find_essential(rpe_handle *h, const float *h_pts1, const float *h_pts2, const int32_t *m, int B,
                                  const double K[9], double *E, uint8_t *mask, int32_t *found, int32_t *info)
{
    if (!h || !h_pts1 || !h_pts2 || !m || !K || B < 1) return rpe_invalid(h, "rpe_find_essential");
    return stage_find_essential(h, "rpe_find_essential", h_pts1, h_pts2, m, B, K, nullptr, nullptr, E, mask, found, info);
}

extern "C" int rpe_find_essential_cameras(rpe_handle *h, const float *h_pts1, const float *h_pts2, const int32_t *m, int B,
                                          const rpe_camera *cam1, const rpe_camera *cam2, double *E, uint8_t *mask,
                                          int32_t *found, int32_t *info)
{
    if (!h || !h_pts1 || !h_pts2 || !m || !cam1 || !cam2 || B < 1) return rpe_invalid(h, "rpe_find_essential_cameras");
    return stage_find_essential(h, "rpe_find_essential_cameras", h_pts1, h_pts2, m, B, nullptr, cam1, cam2, E, mask, found, info);
}

extern "C" int rpe_recover_pose(rpe_handle *h, const double *h_E, const float *h_pts1, const float *h_pts2, const int32_t *m,
                                int B, const double K[9], double *R, double *t, int32_t *inliers)
{
    if (!h || !h_E || !h_pts1 || !h_pts2 || !m || !K || B < 1) return rpe_invalid(h, "rpe_recover_pose");
    return stage_recover_pose(h, "rpe_recover_pose", h_E, h_pts1, h_pts2, m, B, K, nullptr, nullptr, R, t, inliers);
}

extern "C" int rpe_recover_pose_cameras(rpe_handle *h, const double *h_E, const float *h_pts1, const float *h_pts2,
                                        const int32_t *m, int B, const rpe_camera *cam1, const rpe_camera *cam2,
                                        double *R, double *t, int32_t *inliers)
{
    if (!h || !h_E || !h_pts1 || !h_pts2 || !m || !cam1 || !cam2 || B < 1) return rpe_invalid(h, "rpe_recover_pose_cameras");
    return stage_recover_pose(h, "rpe_recover_pose_cameras", h_E, h_pts1, h_pts2, m, B, nullptr, cam1, cam2, R, t, inliers);
}

// ---------------------------------------------------------------- profiling
static const char *kStageNames[RPE_STAGE_COUNT] = {"pyramid", "fast", "nms", "select", "harris", "keypoints",
                                                   "angle", "blur", "describe", "match", "ransac", "pose"};
extern "C" const char *rpe_stage_name(int s) { return (s >= 0 && s < RPE_STAGE_COUNT) ? kStageNames[s] : "?"; }
extern "C" int rpe_set_profiling(rpe_handle *h, int enable)
{
    if (!h) return rpe_invalid(h, "rpe_set_profiling");
    h->profiling = enable != 0; h->ev_valid = false;
    return RPE_OK;
}
extern "C" int rpe_get_stage_ms(rpe_handle *h, float *ms)
{
    if (!h || !ms) return rpe_invalid(h, "rpe_get_stage_ms");
    if (!h->ev_valid) { h->err = "no profiled batch recorded"; return RPE_ERR_INVALID; }
    HIPCHK(h, hipEventSynchronize(h->ev[RPE_STAGE_COUNT]));
    for (int i = 0; i < RPE_STAGE_COUNT; ++i) {
        if (i < h->ev_first) { ms[i] = 0.f; continue; }      // a pair list runs no extraction stage
        HIPCHK(h, hipEventElapsedTime(&ms[i], h->ev[i], h->ev[i + 1]));
    }
    return RPE_OK;
}

// ------------------------------------------------------------------ SIFT stage API
extern "C" int rpe_sift_detect_and_compute(rpe_handle *h, const uint8_t *h_imgs, int n_images,
                                           rpe_sift_keypoint *kps, float *desc, int32_t *counts)
{
    if (!h || !h_imgs || n_images < 1) return rpe_invalid(h, "rpe_sift_detect_and_compute");
    if (h->cfg.feature_method != RPE_FEATURE_SIFT) { h->err = "handle was not created for SIFT"; return RPE_ERR_INVALID; }
    if (n_images > h->n_img_cap) { h->err = "n_images exceeds 2*max_batch"; return RPE_ERR_CAPACITY; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    last_run_end(h);                            // overwrites buffers rpe_fetch_structure reads
    int na, nb;
    int rc = stage_images(h, h_imgs, n_images, na, nb);
    if (rc == RPE_OK) rc = rpe_sift_run(h, h->d_stage1, h->d_stage2, na, nb);
    if (rc) return rc;
    const int kcap = h->lay.kcap;
    std::vector<float> fin((size_t)n_images * kcap * 6);
    std::vector<int> cnt(n_images);
    std::vector<uint8_t> d8(desc ? (size_t)n_images * kcap * 128 : 0);
    if ((rc = rpe_sift_fetch(h, n_images, fin.data(), cnt.data())) != RPE_OK) return rc;
    if (desc) {
        HIPCHK(h, hipMemcpy(d8.data(), h->d_desc, d8.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < d8.size(); ++i) desc[i] = (float)d8[i];       // cv2 returns SIFT descriptors as f32
    }
    for (int i = 0; i < n_images; ++i) {
        if (counts) counts[i] = cnt[i];
        if (!kps) continue;
        for (int k = 0; k < cnt[i]; ++k) {
            const float *f = &fin[((size_t)i * kcap + k) * 6];
            rpe_sift_keypoint &o = kps[(size_t)i * kcap + k];
            int oct; memcpy(&oct, &f[5], 4);
            o.x = f[0] * 0.5f; o.y = f[1] * 0.5f; o.size = f[2] * 0.5f; o.angle = f[3]; o.response = f[4];
            o.octave = (oct & ~255) | ((oct - 1) & 255);                          // firstOctave = -1 (sift.dispatch.cpp)
        }
    }
    return RPE_OK;
}

extern "C" int64_t rpe_sift_debug_gauss(rpe_handle *h, int index, float *out)
{
    if (!h || !h->sift) return 0;
    if (out && rpe_sift_fetch_gauss(h, index, out) != RPE_OK) return -1;
    return rpe_sift_gauss_floats(h);
}

extern "C" int rpe_match_l2(rpe_handle *h, const float *h_desc1, const int32_t *n1, const float *h_desc2, const int32_t *n2, int B,
                            int32_t *qidx, int32_t *tidx, float *dist, int32_t *n_matches)
{
    if (!h || !h_desc1 || !h_desc2 || !n1 || !n2 || B < 1) return rpe_invalid(h, "rpe_match_l2");
    if (h->cfg.norm_type != RPE_NORM_L2) { h->err = "handle was not created for NORM_L2"; return RPE_ERR_INVALID; }
    if (int rc = check_batch(h, B)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    last_run_end(h);                            // overwrites buffers rpe_fetch_structure reads
    std::vector<uint8_t> u;
    if (int rc = l2_desc_bytes(h, h_desc1, n1, h_desc2, n2, B, u)) return rc;
    if (int rc = upload(h, {{h->d_desc, u.data(), u.size()}})) return rc;
    return stage_match_run(h, true, n1, n2, B, qidx, tidx, dist, n_matches);
}
