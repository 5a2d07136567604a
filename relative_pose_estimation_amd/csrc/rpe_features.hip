// rpe_features.hip -- the first-use features of the C-ABI (include/rpe_amd.h): entry points that create their device buffers on
// first use, one record of the handle each (rpe_internal.h), and keep nothing.  No kernel; the shared helpers: rpe_host.h.
#include "rpe_internal.h"
#include "rpe_host.h"
#include "graph_plan.h"
#include <string.h>

// iters and threshold_px of the calls that run a RANSAC of their own behind the last run (homography, link poses)
static int homography_check(rpe_handle *h, const char *who, int iters, double threshold_px)
{
    if (iters < 1 || iters > h->cfg.ransac_max_iters) return rpe_invalid(h, who, "iters must be 1 ... ransac_max_iters");
    return check_positive(h, who, "threshold_px", threshold_px);
}

// The argument head of the calls over links (rpe_scale_links, rpe_link_poses, rpe_link_bundles): every check on the host first (the kept
// pair table of a list, the rule of a stream), then the structure kernels when the per-match buffers do not hold their
// results for the whole run, and the link table on its way to link.links.  L == 0 passes the checks and does nothing more.
static int links_begin(rpe_handle *h, const char *who, int L, const int32_t *pair_a, const int32_t *pair_b, const int32_t *side, int min_shared)
{
    const std::string w(who);
    if (L < 0 || min_shared < 1 || (L > 0 && (!pair_a || !pair_b || !side))) { h->err = w + ": L < 0, min_shared < 1 or a null link array"; return RPE_ERR_INVALID; }
    int rc = last_run_gate(h, who, h->last.pairs, NEED_UNCHUNKED | NEED_PER_MATCH | NEED_TABLE);
    if (rc) return rc;
    const RpeLastRun &l = h->last;
    const bool list = l.kind == RpeLastRun::LIST;
    if (!list && l.run.feat.img2_base != 1) { h->err = w + ": the pairs of a batch share no frame (links join the pairs of a stream or of a pair list)"; return RPE_ERR_INVALID; }
    if (L > rpe_link_capacity(h)) { h->err = w + ": more than 4*max_batch links in one call"; return RPE_ERR_CAPACITY; }
    std::vector<RpeLink> &tbl = h->link.tab;                // outlives the call: the upload below is asynchronous
    tbl.assign((size_t)L, RpeLink{0, 0, 0, 0});
    for (int i = 0; i < L; ++i) {
        const int a = pair_a[i], b = pair_b[i], s = side[i];
        const char *bad = nullptr;
        if (a < 0 || a >= l.pairs || b < 0 || b >= l.pairs) bad = ": pair index outside the last run";
        else if (a == b) bad = ": a link joins two different pairs";
        else if (s < 0 || s > 3) bad = ": side must be 0 ... 3";
        else if (list ? l.tab[(size_t)2 * a + (s & 1)] != l.tab[(size_t)2 * b + (s >> 1)] : a + (s & 1) != b + (s >> 1))
            bad = ": the two pairs do not share the frame the link names";
        if (bad) { h->err = w + bad; return RPE_ERR_INVALID; }
        tbl[(size_t)i] = {a, b, s, 0};
    }
    if (L == 0) return RPE_OK;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DM_ONCE(h, h->link.links, (size_t)rpe_link_capacity(h));
    if ((rc = last_run_structure(h, l.pairs, false)) != RPE_OK) return rc;
    return upload(h, {{h->link.links, tbl.data(), sizeof(RpeLink) * (size_t)L}});
}

static int scale_links_alloc(rpe_handle *h)
{
    const size_t lcap = (size_t)rpe_link_capacity(h);
    return rpe_bufset_fit(h, h->link.set, {buf_piece(h->link.stats, lcap * 3), buf_piece(h->link.n, lcap), buf_piece(h->link.code, lcap)});
}

extern "C" int rpe_scale_links(rpe_handle *h, int L, const int32_t *pair_a, const int32_t *pair_b, const int32_t *side,
                               int min_shared, double *stats, int32_t *n_shared, int32_t *code)
{
    if (!h) return rpe_invalid(h, "rpe_scale_links");
    int rc = links_begin(h, "rpe_scale_links", L, pair_a, pair_b, side, min_shared);
    if (rc != RPE_OK || L == 0) return rc;
    if ((rc = scale_links_alloc(h)) != RPE_OK) return rc;
    rpe_launch_scale_links(h, L, min_shared);
    HIPCHK(h, hipGetLastError());
    return fetch(h, {{stats, h->link.stats, sizeof(double) * 3 * (size_t)L}, {n_shared, h->link.n, sizeof(int) * (size_t)L},
                     {code, h->link.code, sizeof(int) * (size_t)L}});
}

// lp.corr: 0 bytes, so null, on handles whose kernel keeps the correspondence lists in LDS
static int link_poses_alloc(rpe_handle *h)
{
    const size_t lcap = (size_t)rpe_link_capacity(h), mm = (size_t)h->cfg.max_matches;
    return rpe_bufset_fit(h, h->lp.set,
                          {buf_piece(h->lp.R, lcap * 9), buf_piece(h->lp.t, lcap * 3), buf_piece(h->lp.rms, lcap * 2),
                           buf_piece(h->lp.counts, lcap * 2), buf_piece(h->lp.info, lcap * 4), buf_piece(h->lp.mask, lcap * mm),
                           buf_piece(h->lp.corr, rpe_link_poses_in_lds(h) ? 0 : lcap * RPE_LINK_POSE_CORR_DOUBLES * mm)});
}

// rpe_link_poses: the links' argument head, its own three checks (all before anything is launched), the buffers on first
// use, one kernel, one fetch.  Nothing of the run is written.
extern "C" int rpe_link_poses(rpe_handle *h, int L, const int32_t *pair_a, const int32_t *pair_b, const int32_t *side,
                              int iters, double threshold_px, int min_shared, int refine_iters,
                              double *R, double *t, uint8_t *mask, int32_t *counts, int32_t *info, double *rms)
{
    if (!h) return rpe_invalid(h, "rpe_link_poses");
    int rc = homography_check(h, "rpe_link_poses", iters, threshold_px);
    if (rc) return rc;
    if (refine_iters < 0 || refine_iters > 100) return rpe_invalid(h, "rpe_link_poses", "refine_iters must be 0 ... 100");
    rc = links_begin(h, "rpe_link_poses", L, pair_a, pair_b, side, min_shared);
    if (rc != RPE_OK || L == 0) return rc;
    if ((rc = link_poses_alloc(h)) != RPE_OK) return rc;
    rpe_launch_link_poses(h, h->last.run, L, iters, threshold_px, min_shared, refine_iters);
    HIPCHK(h, hipGetLastError());
    const size_t n = (size_t)L, mm = (size_t)h->cfg.max_matches;
    return fetch(h, {{R, h->lp.R, sizeof(double) * 9 * n}, {t, h->lp.t, sizeof(double) * 3 * n}, {mask, h->lp.mask, n * mm},
                     {counts, h->lp.counts, sizeof(int) * 2 * n}, {info, h->lp.info, sizeof(int) * 4 * n}, {rms, h->lp.rms, sizeof(double) * 2 * n}});
}

// link bundles: the buffers of both forms; ba.state: 0 bytes, so null, on handles whose kernel keeps the point state in LDS
static int bundle_alloc(rpe_handle *h)
{
    const size_t lcap = (size_t)rpe_link_capacity(h), mm = (size_t)h->cfg.max_matches;
    return rpe_bufset_fit(h, h->ba.set,
                          {buf_piece(h->ba.views, lcap * mm), buf_piece(h->ba.obs, lcap * mm * RPE_BUNDLE_OBS_DOUBLES), buf_piece(h->ba.points, lcap * mm * 3),
                           buf_piece(h->ba.pose0, lcap * RPE_BUNDLE_POSE_DOUBLES), buf_piece(h->ba.focal, lcap * 2), buf_piece(h->ba.n, lcap), buf_piece(h->ba.pre, lcap),
                           buf_piece(h->ba.Rin, lcap * 9), buf_piece(h->ba.tin, lcap * 3),
                           buf_piece(h->ba.Ra, lcap * 9), buf_piece(h->ba.ta, lcap * 3), buf_piece(h->ba.Rb, lcap * 9), buf_piece(h->ba.tb, lcap * 3),
                           buf_piece(h->ba.counts, lcap * 2), buf_piece(h->ba.info, lcap * 4), buf_piece(h->ba.rms, lcap * 2),
                           buf_piece(h->ba.state, rpe_bundles_in_lds(h) ? 0 : lcap * mm * RPE_BUNDLE_STATE_DOUBLES)});
}

static int bundle_fetch(rpe_handle *h, size_t n, double *R_a, double *t_a, double *R_b, double *t_b, double *points, uint8_t *views,
                        int32_t *counts, int32_t *info, double *rms)
{
    const size_t mm = (size_t)h->cfg.max_matches;
    return fetch(h, {{R_a, h->ba.Ra, sizeof(double) * 9 * n}, {t_a, h->ba.ta, sizeof(double) * 3 * n}, {R_b, h->ba.Rb, sizeof(double) * 9 * n},
                     {t_b, h->ba.tb, sizeof(double) * 3 * n}, {points, h->ba.points, sizeof(double) * 3 * n * mm}, {views, h->ba.views, n * mm},
                     {counts, h->ba.counts, sizeof(int) * 2 * n}, {info, h->ba.info, sizeof(int) * 4 * n}, {rms, h->ba.rms, sizeof(double) * 2 * n}});
}

// rpe_link_bundles: its own checks and the links' argument head (all before anything is launched), the buffers on first
// use, the poses of pair b up, two kernels, one fetch.  Nothing of the run is written.
extern "C" int rpe_link_bundles(rpe_handle *h, int L, const int32_t *pair_a, const int32_t *pair_b, const int32_t *side,
                                const double *R0, const double *t0, double threshold_px, int min_shared, int max_iters,
                                double *R_a, double *t_a, double *R_b, double *t_b, double *points, uint8_t *views,
                                int32_t *counts, int32_t *info, double *rms)
{
    if (!h) return rpe_invalid(h, "rpe_link_bundles");
    if (int rc = check_positive(h, "rpe_link_bundles", "threshold_px", threshold_px)) return rc;
    if (max_iters < 1 || max_iters > 100) return rpe_invalid(h, "rpe_link_bundles", "max_iters must be 1 ... 100");
    if ((R0 == nullptr) != (t0 == nullptr) || (L > 0 && !R0)) return rpe_invalid(h, "rpe_link_bundles", "R0 and t0 must both be given");
    const size_t n = (size_t)std::max(L, 0);
    if (R0 && (!all_finite(R0, 9 * n) || !all_finite(t0, 3 * n))) return rpe_invalid(h, "rpe_link_bundles", "a pose has a non-finite entry");
    int rc = links_begin(h, "rpe_link_bundles", L, pair_a, pair_b, side, min_shared);
    if (rc != RPE_OK || L == 0) return rc;
    if ((rc = bundle_alloc(h)) != RPE_OK) return rc;
    if ((rc = upload(h, {{h->ba.Rin, R0, sizeof(double) * 9 * n}, {h->ba.tin, t0, sizeof(double) * 3 * n}})) != RPE_OK) return rc;
    rpe_launch_bundle_gather(h, h->last.run, L, threshold_px);
    rpe_launch_bundle(h, L, min_shared, max_iters, true);
    HIPCHK(h, hipGetLastError());
    // the wait also covers the upload: the poses have left the caller's arrays
    return bundle_fetch(h, n, R_a, t_a, R_b, t_b, points, views, counts, info, rms);
}

// rpe_bundle_three_view: the problems' arrays packed on the host as the gather kernel leaves them, one kernel, one fetch
extern "C" int rpe_bundle_three_view(rpe_handle *h, int B, const int32_t *n, const double *obs_s, const double *obs_a,
                                     const double *obs_c, const uint8_t *has_c, const double *X0, const double *Ra0, const double *ta0,
                                     const double *Rc0, const double *tc0, double f_a, double f_c, int max_iters,
                                     double *R_a, double *t_a, double *R_c, double *t_c, double *points, uint8_t *views,
                                     int32_t *counts, int32_t *info, double *rms)
{
    if (!h || !n || !obs_s || !obs_a || !obs_c || !has_c || !X0 || !Ra0 || !ta0 || !Rc0 || !tc0 || B < 1) return rpe_invalid(h, "rpe_bundle_three_view");
    if (int rc = check_batch(h, B)) return rc;
    if (max_iters < 1 || max_iters > 100) return rpe_invalid(h, "rpe_bundle_three_view", "max_iters must be 1 ... 100");
    if (!std::isfinite(f_a) || !(f_a > 0.) || !std::isfinite(f_c) || !(f_c > 0.)) return rpe_invalid(h, "rpe_bundle_three_view", "f_a and f_c must be finite and > 0");
    int rc = check_match_counts(h, n, B);
    if (rc) return rc;
    const size_t nb = (size_t)B, mm = (size_t)h->cfg.max_matches, OB = RPE_BUNDLE_OBS_DOUBLES, PO = RPE_BUNDLE_POSE_DOUBLES;
    if (!all_finite(Ra0, 9 * nb) || !all_finite(ta0, 3 * nb) || !all_finite(Rc0, 9 * nb) || !all_finite(tc0, 3 * nb))
        return rpe_invalid(h, "rpe_bundle_three_view", "a pose has a non-finite entry");
    std::vector<uint8_t> vw(nb * mm, 0);
    std::vector<double> ob(nb * mm * OB, 0.), x0(nb * mm * 3, 0.), pose(nb * PO), foc(nb * 2);
    std::vector<int> pre(nb, RPE_BUNDLE_OK);
    for (size_t p = 0; p < nb; ++p) {
        for (size_t i = 0; i < (size_t)n[p]; ++i) {
            const size_t k = p * mm + i;
            vw[k] = has_c[k] ? 3 : 1;
            ob[k * OB] = obs_s[k * 2]; ob[k * OB + 1] = obs_s[k * 2 + 1]; ob[k * OB + 2] = obs_a[k * 2]; ob[k * OB + 3] = obs_a[k * 2 + 1];
            if (has_c[k]) { ob[k * OB + 4] = obs_c[k * 2]; ob[k * OB + 5] = obs_c[k * 2 + 1]; }
            for (int e = 0; e < 3; ++e) x0[k * 3 + e] = X0[k * 3 + e];
        }
        for (int e = 0; e < 9; ++e) { pose[p * PO + e] = Ra0[p * 9 + e]; pose[p * PO + 12 + e] = Rc0[p * 9 + e]; }
        for (int e = 0; e < 3; ++e) { pose[p * PO + 9 + e] = ta0[p * 3 + e]; pose[p * PO + 21 + e] = tc0[p * 3 + e]; }
        foc[p * 2] = f_a; foc[p * 2 + 1] = f_c;
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = bundle_alloc(h)) != RPE_OK) return rc;
    if ((rc = upload(h, {{h->ba.views, vw.data(), vw.size()}, {h->ba.obs, ob.data(), sizeof(double) * ob.size()},
                         {h->ba.points, x0.data(), sizeof(double) * x0.size()}, {h->ba.pose0, pose.data(), sizeof(double) * pose.size()},
                         {h->ba.focal, foc.data(), sizeof(double) * foc.size()}, {h->ba.pre, pre.data(), sizeof(int) * nb},
                         {h->ba.n, n, sizeof(int) * nb}})) != RPE_OK) return rc;
    rpe_launch_bundle(h, B, 1, max_iters, false);
    HIPCHK(h, hipGetLastError());
    // the wait also covers the uploads: the staging vectors live until it returns
    return bundle_fetch(h, nb, R_a, t_a, R_c, t_c, points, views, counts, info, rms);
}

// ---- multi-view tracks (rpe_build_tracks / rpe_tracks_from_matches)
// the buffers of both forms: per match slot, then per node and per frame of this call's n_frames
static int tracks_alloc(rpe_handle *h, int n_frames)
{
    const size_t MB = (size_t)h->cfg.max_batch, cap = MB * h->cfg.max_matches;
    const int N = n_frames * h->lay.kcap;
    return rpe_bufset_fit(h, h->tk.set,
                          {buf_piece(h->tk.eflag, cap), buf_piece(h->tk.edge, cap), buf_piece(h->tk.use, MB),
                           buf_piece(h->tk.mtrack, cap), buf_piece(h->tk.q, cap), buf_piece(h->tk.t, cap), buf_piece(h->tk.m, MB),
                           buf_piece(h->tk.counts, 8), buf_piece(h->tk.tstart, cap + 1), buf_piece(h->tk.oframe, 2 * cap), buf_piece(h->tk.okp, 2 * cap),
                           buf_piece(h->tk.oxy, 2 * cap), buf_piece(h->tk.pts1, cap), buf_piece(h->tk.pts2, cap), buf_piece(h->tk.frames, MB),
                           buf_piece(h->tk.node, (size_t)RPE_TRACK_NODE_WORDS * N), buf_piece(h->tk.partial, (size_t)rpe_track_scan_blocks(N)),
                           buf_piece(h->tk.seen, (size_t)n_frames)});
}

// min_len, and the node ids and edge ids of n_frames frames must fit an int.  frames_what: the refusal in the caller's terms
static int tracks_check(rpe_handle *h, const char *who, int n_frames, int min_len, const char *frames_what)
{
    if (min_len < 2) return rpe_invalid(h, who, "min_len must be >= 2");
    if (n_frames < 1 || (long long)n_frames * h->lay.kcap >= (1LL << 31)) return rpe_invalid(h, who, frames_what);
    if ((long long)h->cfg.max_batch * h->cfg.max_matches >= (1LL << 30)) return rpe_invalid(h, who, "max_batch * max_matches must be < 2^30");
    return RPE_OK;
}

// the frame table up, the kernels, counts first and then the used prefixes
static int tracks_run(rpe_handle *h, RpeTrackJob job, int32_t *counts, int32_t *track_start, int32_t *obs_frame, int32_t *obs_kp,
                      float *obs_xy, int32_t *match_track)
{
    const size_t P = (size_t)job.P;
    if (int rc = upload(h, {{h->tk.frames, h->tk.frame_tab.data(), sizeof(int2) * P}})) return rc;
    job.frames = h->tk.frames;
    rpe_launch_tracks(h, job);
    HIPCHK(h, hipGetLastError());
    int32_t c[6];
    if (int rc = fetch(h, {{c, h->tk.counts, sizeof(c)}})) return rc;
    if (counts) memcpy(counts, c, sizeof(c));
    const size_t nt = (size_t)c[0], no = (size_t)c[1];
    return fetch(h, {{track_start, h->tk.tstart, sizeof(int) * (nt + 1)}, {obs_frame, h->tk.oframe, sizeof(int) * no},
                     {obs_kp, h->tk.okp, sizeof(int) * no}, {obs_xy, h->tk.oxy, sizeof(float2) * no},
                     {match_track, h->tk.mtrack, sizeof(int) * P * h->cfg.max_matches}});
}

// rpe_build_tracks: every check on the host first, the buffers, the structure kernels when the rule reads masks that are
// not current, the kernels, the fetch.  Nothing of the run is written.
extern "C" int rpe_build_tracks(rpe_handle *h, const uint8_t *use_pair, int edge_rule, int min_len,
                                int32_t *counts, int32_t *track_start, int32_t *obs_frame, int32_t *obs_kp, float *obs_xy,
                                int32_t *match_track)
{
    if (!h) return rpe_invalid(h, "rpe_build_tracks");
    if (edge_rule < RPE_TRACK_EDGES_USABLE || edge_rule > RPE_TRACK_EDGES_ALL) return rpe_invalid(h, "rpe_build_tracks", "edge_rule must be 0 ... 2");
    int rc = last_run_gate(h, "rpe_build_tracks", h->last.pairs, NEED_UNCHUNKED | NEED_PER_MATCH | NEED_TABLE);
    if (rc) return rc;
    const RpeLastRun &l = h->last;
    const bool list = l.kind == RpeLastRun::LIST;
    // a batch of one pair has img2_base == 1 like a stream of two frames: it is served as that stream (the header says so)
    if (!list && l.run.feat.img2_base != 1) return rpe_invalid(h, "rpe_build_tracks", "the pairs of a batch share no frame (links join the pairs of a stream or of a pair list)");
    const int P = l.pairs, n_frames = list ? h->fs.cap : P + 1;
    if ((rc = tracks_check(h, "rpe_build_tracks", n_frames, min_len,
                           "the frames of the run (a pair list: the store's capacity) times the keypoint capacity must be < 2^31")) != RPE_OK) return rc;
    h->tk.frame_tab.resize((size_t)2 * P);
    for (int p = 0; p < P; ++p) {
        h->tk.frame_tab[(size_t)2 * p] = list ? l.tab[(size_t)2 * p] : p;
        h->tk.frame_tab[(size_t)2 * p + 1] = list ? l.tab[(size_t)2 * p + 1] : p + 1;
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = tracks_alloc(h, n_frames)) != RPE_OK) return rc;
    if (edge_rule != RPE_TRACK_EDGES_ALL && (rc = last_run_structure(h, P, false)) != RPE_OK) return rc;
    if ((rc = upload(h, {{h->tk.use, use_pair, (size_t)P}})) != RPE_OK) return rc;
    const RpeTrackJob job = {P, n_frames, edge_rule, min_len, nullptr, h->d_m_n, h->d_m_q, h->d_m_t, use_pair ? h->tk.use : nullptr, nullptr,
                             h->d_status, h->d_mask, h->d_pose_mask, h->d_pts1, h->d_pts2};
    // the first wait also covers the uploads: use_pair has left the caller's array
    return tracks_run(h, job, counts, track_start, obs_frame, obs_kp, obs_xy, match_track);
}

// rpe_tracks_from_matches: the caller's lists into the track buffers, the same kernels under RPE_TRACK_EDGES_ALL.  Neither
// the workspace nor the record of the last run is touched.
extern "C" int rpe_tracks_from_matches(rpe_handle *h, int P, int n_frames, const int32_t *frame1, const int32_t *frame2, const int32_t *m,
                                       const int32_t *qidx, const int32_t *tidx, const uint8_t *edge, const float *pts1, const float *pts2,
                                       int min_len, int32_t *counts, int32_t *track_start, int32_t *obs_frame, int32_t *obs_kp,
                                       float *obs_xy, int32_t *match_track)
{
    const char *who = "rpe_tracks_from_matches";
    if (!h || P < 0 || (P > 0 && (!frame1 || !frame2 || !m || !qidx || !tidx))) return rpe_invalid(h, who);
    if (int rc = check_batch(h, P)) return rc;
    int rc = tracks_check(h, who, n_frames, min_len, "n_frames must be >= 1 and n_frames * keypoint capacity < 2^31");
    if (rc) return rc;
    if ((pts1 == nullptr) != (pts2 == nullptr)) return rpe_invalid(h, who, "pts1 and pts2 must both be given or both be NULL");
    if ((rc = check_match_counts(h, m, P)) != RPE_OK) return rc;
    const size_t mm = (size_t)h->cfg.max_matches;
    const int KC = h->lay.kcap;
    for (int p = 0; p < P; ++p) {
        if (frame1[p] < 0 || frame1[p] >= n_frames || frame2[p] < 0 || frame2[p] >= n_frames) return rpe_invalid(h, who, "a frame index outside 0 ... n_frames - 1");
        for (size_t i = 0; i < (size_t)m[p]; ++i) {
            const int q = qidx[p * mm + i], t = tidx[p * mm + i];
            if (q < 0 || q >= KC || t < 0 || t >= KC) return rpe_invalid(h, who, "a keypoint index outside 0 ... keypoint capacity - 1");
        }
    }
    if (P == 0) {
        if (counts) memset(counts, 0, sizeof(int32_t) * 6);
        if (track_start) track_start[0] = 0;
        return RPE_OK;
    }
    h->tk.frame_tab.resize((size_t)2 * P);
    for (int p = 0; p < P; ++p) { h->tk.frame_tab[(size_t)2 * p] = frame1[p]; h->tk.frame_tab[(size_t)2 * p + 1] = frame2[p]; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = tracks_alloc(h, n_frames)) != RPE_OK) return rc;
    const size_t n = (size_t)P * mm;
    if ((rc = upload(h, {{h->tk.m, m, sizeof(int) * (size_t)P}, {h->tk.q, qidx, sizeof(int) * n}, {h->tk.t, tidx, sizeof(int) * n},
                         {h->tk.edge, edge, n}, {h->tk.pts1, pts1, sizeof(float2) * n}, {h->tk.pts2, pts2, sizeof(float2) * n}})) != RPE_OK) return rc;
    const RpeTrackJob job = {P, n_frames, RPE_TRACK_EDGES_ALL, min_len, nullptr, h->tk.m, h->tk.q, h->tk.t, nullptr, edge ? h->tk.edge : nullptr,
                             nullptr, nullptr, nullptr, pts1 ? h->tk.pts1 : nullptr, pts1 ? h->tk.pts2 : nullptr};
    // the first wait also covers the uploads: the lists have left the caller's arrays
    return tracks_run(h, job, counts, track_start, obs_frame, obs_kp, obs_xy, match_track);
}

// refined poses: device buffers on first use, launch, fetch
static int refine_alloc(rpe_handle *h)
{
    const size_t MB = (size_t)h->cfg.max_batch;
    return rpe_bufset_fit(h, h->ref.set,
                          {buf_piece(h->ref.R, MB * 9), buf_piece(h->ref.t, MB * 3), buf_piece(h->ref.rms, MB * 2),
                           buf_piece(h->ref.R0, MB * 9), buf_piece(h->ref.t0, MB * 3), buf_piece(h->ref.inl, MB), buf_piece(h->ref.info, MB * 4)});
}

static int refine_run(rpe_handle *h, const RpeRun &r, int max_iters, bool from_batch, double *R, double *t, int32_t *inliers,
                      int32_t *info, double *rms)
{
    const int B = r.pairs;
    rpe_launch_refine(h, r, max_iters, from_batch);
    HIPCHK(h, hipGetLastError());
    return fetch(h, {{R, h->ref.R, sizeof(double) * 9 * B}, {t, h->ref.t, sizeof(double) * 3 * B}, {inliers, h->ref.inl, sizeof(int) * B},
                     {info, h->ref.info, sizeof(int) * 4 * B}, {rms, h->ref.rms, sizeof(double) * 2 * B}});
}

extern "C" int rpe_refine_poses(rpe_handle *h, int B, int max_iters, double *R, double *t, int32_t *inliers,
                                int32_t *info, double *rms)
{
    if (!h || B < 1 || B > h->cfg.max_batch) return rpe_invalid(h, "rpe_refine_poses");
    if (max_iters < 1 || max_iters > 100) return rpe_invalid(h, "rpe_refine_poses", "max_iters must be 1 ... 100");
    int rc = last_run_gate(h, "rpe_refine_poses", B, NEED_UNCHUNKED | NEED_PER_MATCH | NEED_COUNT);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = refine_alloc(h)) != RPE_OK) return rc;
    return refine_run(h, last_run_first(h, B), max_iters, true, R, t, inliers, info, rms);
}

// ---------------------------------------------------------------- guided matching
// rpe_guided_matches / rpe_match_hamming_guided and their L2 forms rpe_guided_matches_l2 / rpe_match_l2_guided (NOT in the
// reference): the mutual-nearest-neighbour match again, among the keypoint pairs that pass the Sampson gate of a pose.
// Results go to the gm.* buffers (gm.d: int32 Hamming or f32 L2 distances); nothing of the run's results is written.
// norm: the norm the entry point serves; max_distance: an integer 0 ... 256 for Hamming, >= 0 or +inf for L2.
static int guided_check(rpe_handle *h, const char *who, int norm, int B, const double *R, const double *t, double gate_px, double max_distance)
{
    const std::string w(who);
    const bool l2 = norm == RPE_NORM_L2;
    if (h->cfg.norm_type != norm) {
        h->err = w + (l2 ? ": L2 handles only (RPE_NORM_L2: SIFT, or ORB bytes under L2)" : ": Hamming handles only (ORB with RPE_NORM_HAMMING)");
        return RPE_ERR_INVALID;
    }
    if (int rc = check_positive(h, who, "gate_px", gate_px)) return rc;
    if (l2 ? !(max_distance >= 0.) : (max_distance < 0 || max_distance > 256)) {
        h->err = w + (l2 ? ": max_distance must be >= 0 (+inf: no bound)" : ": max_distance must be 0 ... 256");
        return RPE_ERR_INVALID;
    }
    if ((R == nullptr) != (t == nullptr)) { h->err = w + ": R and t must both be given or both be NULL"; return RPE_ERR_INVALID; }
    if (R && (!all_finite(R, (size_t)9 * B) || !all_finite(t, (size_t)3 * B))) { h->err = w + ": a pose has a non-finite entry"; return RPE_ERR_INVALID; }
    return RPE_OK;
}

static int guided_alloc(rpe_handle *h)
{
    const size_t MB = (size_t)h->cfg.max_batch, cap = MB * h->cfg.max_matches;
    return rpe_bufset_fit(h, h->gm.set,
                          {buf_piece(h->gm.q, cap), buf_piece(h->gm.t, cap), buf_piece(h->gm.d, cap), buf_piece(h->gm.n, MB),
                           buf_piece(h->gm.pts1, cap), buf_piece(h->gm.pts2, cap), buf_piece(h->gm.R, MB * 9), buf_piece(h->gm.tr, MB * 3), buf_piece(h->gm.thr2, MB),
                           buf_piece(h->gm.rec, MB * RPE_GUIDED_SIDES * h->lay.kcap)});
}

// poses up (R == nullptr: the run's own, and its status words), launch, fetch
static int guided_run(rpe_handle *h, const RpeRun &r, const double *R, const double *t, double gate_px, double max_distance,
                      int32_t *qidx, int32_t *tidx, void *dist, float *pts1, float *pts2, int32_t *n_matches)
{
    const size_t B = (size_t)r.pairs, n = B * h->cfg.max_matches;
    if (int rc = upload(h, {{h->gm.R, R, sizeof(double) * 9 * B}, {h->gm.tr, t, sizeof(double) * 3 * B}})) return rc;
    const double *d_R = R ? h->gm.R : h->d_R, *d_t = R ? h->gm.tr : h->d_t;
    const int *d_status = R ? (const int *)nullptr : (const int *)h->d_status;
    if (h->cfg.norm_type == RPE_NORM_L2) rpe_launch_guided_l2(h, r, d_R, d_t, d_status, gate_px, max_distance);
    else rpe_launch_guided(h, r, d_R, d_t, d_status, gate_px, (int)max_distance);
    HIPCHK(h, hipGetLastError());
    // the wait also covers the upload: the poses have left the caller's arrays
    return fetch(h, {{qidx, h->gm.q, sizeof(int) * n}, {tidx, h->gm.t, sizeof(int) * n}, {dist, h->gm.d, sizeof(int) * n},
                     {pts1, h->gm.pts1, sizeof(float2) * n}, {pts2, h->gm.pts2, sizeof(float2) * n}, {n_matches, h->gm.n, sizeof(int) * B}});
}

// the run form of either norm: over the first B pairs of the last run
static int guided_last_run(rpe_handle *h, const char *who, int norm, int B, const double *R, const double *t, double gate_px, double max_distance,
                           int32_t *qidx, int32_t *tidx, void *dist, float *pts1, float *pts2, int32_t *n_matches)
{
    int rc = guided_check(h, who, norm, B, R, t, gate_px, max_distance);
    if (rc) return rc;
    // the features of the run must still be where it read them (a stage call or a put overwrote the workspace's) and, under
    // the run's own poses, d_R / d_t / d_status its results
    rc = last_run_gate(h, who, B, NEED_UNCHUNKED | NEED_PER_MATCH | NEED_COUNT | NEED_TABLE);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = guided_alloc(h)) != RPE_OK) return rc;
    return guided_run(h, last_run_first(h, B), R, t, gate_px, max_distance, qidx, tidx, dist, pts1, pts2, n_matches);
}

extern "C" int rpe_guided_matches(rpe_handle *h, int B, const double *R, const double *t, double gate_px, int max_distance,
                                  int32_t *qidx, int32_t *tidx, int32_t *dist, float *pts1, float *pts2, int32_t *n_matches)
{
    if (!h || B < 1 || B > h->cfg.max_batch) return rpe_invalid(h, "rpe_guided_matches");
    return guided_last_run(h, "rpe_guided_matches", RPE_NORM_HAMMING, B, R, t, gate_px, max_distance, qidx, tidx, dist, pts1, pts2, n_matches);
}

extern "C" int rpe_guided_matches_l2(rpe_handle *h, int B, const double *R, const double *t, double gate_px, double max_distance,
                                     int32_t *qidx, int32_t *tidx, float *dist, float *pts1, float *pts2, int32_t *n_matches)
{
    if (!h || B < 1 || B > h->cfg.max_batch) return rpe_invalid(h, "rpe_guided_matches_l2");
    return guided_last_run(h, "rpe_guided_matches_l2", RPE_NORM_L2, B, R, t, gate_px, max_distance, qidx, tidx, dist, pts1, pts2, n_matches);
}

// tail of the stage forms (descriptors of pair p uploaded to workspace slots p and B + p): points, counts, match, fetch
static int guided_stage_run(rpe_handle *h, const float *h_pts1, const int32_t *n1, const float *h_pts2, const int32_t *n2, int B,
                            const double *R, const double *t, double gate_px, double max_distance,
                            int32_t *qidx, int32_t *tidx, void *dist, int32_t *n_matches)
{
    const size_t kcap = (size_t)h->lay.kcap;
    if (int rc = upload(h, {{h->d_kp_pt, h_pts1, sizeof(float2) * kcap * B}, {h->d_kp_pt + kcap * B, h_pts2, sizeof(float2) * kcap * B}})) return rc;
    if (int rc = upload_counts(h, n1, n2, B)) return rc;
    return guided_run(h, rpe_run_batch(h, B), R, t, gate_px, max_distance, qidx, tidx, dist, nullptr, nullptr, n_matches);
}

extern "C" int rpe_match_hamming_guided(rpe_handle *h, const uint8_t *h_desc1, const float *h_pts1, const int32_t *n1,
                                        const uint8_t *h_desc2, const float *h_pts2, const int32_t *n2, int B,
                                        const double K[9], const double *R, const double *t, double gate_px, int max_distance,
                                        int32_t *qidx, int32_t *tidx, int32_t *dist, int32_t *n_matches)
{
    if (!h || !h_desc1 || !h_pts1 || !n1 || !h_desc2 || !h_pts2 || !n2 || !K || !R || !t || B < 1) return rpe_invalid(h, "rpe_match_hamming_guided");
    if (int rc = check_batch(h, B)) return rc;
    int rc = guided_check(h, "rpe_match_hamming_guided", RPE_NORM_HAMMING, B, R, t, gate_px, max_distance);
    if (rc) return rc;
    if ((rc = check_desc_counts(h, n1, B)) != RPE_OK || (rc = check_desc_counts(h, n2, B)) != RPE_OK) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = guided_alloc(h)) != RPE_OK) return rc;
    last_run_end(h);                            // overwrites the workspace's features
    if ((rc = set_K(h, K)) != RPE_OK) return rc;
    // pair p on the workspace slots (p, B + p), like every stage call
    if ((rc = upload_descriptors(h, h_desc1, h_desc2, B)) != RPE_OK) return rc;
    return guided_stage_run(h, h_pts1, n1, h_pts2, n2, B, R, t, gate_px, max_distance, qidx, tidx, dist, n_matches);
}

extern "C" int rpe_match_l2_guided(rpe_handle *h, const float *h_desc1, const float *h_pts1, const int32_t *n1,
                                   const float *h_desc2, const float *h_pts2, const int32_t *n2, int B,
                                   const double K[9], const double *R, const double *t, double gate_px, double max_distance,
                                   int32_t *qidx, int32_t *tidx, float *dist, int32_t *n_matches)
{
    if (!h || !h_desc1 || !h_pts1 || !n1 || !h_desc2 || !h_pts2 || !n2 || !K || !R || !t || B < 1) return rpe_invalid(h, "rpe_match_l2_guided");
    if (int rc = check_batch(h, B)) return rc;
    int rc = guided_check(h, "rpe_match_l2_guided", RPE_NORM_L2, B, R, t, gate_px, max_distance);
    if (rc) return rc;
    std::vector<uint8_t> u;
    if ((rc = l2_desc_bytes(h, h_desc1, n1, h_desc2, n2, B, u)) != RPE_OK) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = guided_alloc(h)) != RPE_OK) return rc;
    last_run_end(h);                            // overwrites the workspace's features
    if ((rc = set_K(h, K)) != RPE_OK) return rc;
    if ((rc = upload(h, {{h->d_desc, u.data(), u.size()}})) != RPE_OK) return rc;
    return guided_stage_run(h, h_pts1, n1, h_pts2, n2, B, R, t, gate_px, max_distance, qidx, tidx, dist, n_matches);   // waits: u is read by then
}

// ---------------------------------------------------------------- homography / rotation-only
// rpe_pair_homographies / rpe_find_homography (NOT in the reference): a homography by RANSAC over the matches of a pair,
// the rotation fitted to its inliers and the three inlier counts.  Results go to the hg.* buffers; nothing of the run
// is written.
static int homography_alloc(rpe_handle *h)
{
    const size_t MB = (size_t)h->cfg.max_batch;
    return rpe_bufset_fit(h, h->hg.set,
                          {buf_piece(h->hg.H, MB * 9), buf_piece(h->hg.R, MB * 9), buf_piece(h->hg.counts, MB * 3), buf_piece(h->hg.info, MB * 4),
                           buf_piece(h->hg.mask, MB * h->cfg.max_matches)});
}

static int homography_run(rpe_handle *h, const RpeRun &r, int iters, double threshold_px, bool from_batch, double *H, double *R_rot,
                          uint8_t *mask, int32_t *counts, int32_t *info)
{
    const size_t B = (size_t)r.pairs;
    rpe_launch_homography(h, r, iters, threshold_px, from_batch);
    HIPCHK(h, hipGetLastError());
    return fetch(h, {{H, h->hg.H, sizeof(double) * 9 * B}, {R_rot, h->hg.R, sizeof(double) * 9 * B}, {mask, h->hg.mask, B * h->cfg.max_matches},
                     {counts, h->hg.counts, sizeof(int) * 3 * B}, {info, h->hg.info, sizeof(int) * 4 * B}});
}

extern "C" int rpe_pair_homographies(rpe_handle *h, int B, int iters, double threshold_px, double *H, double *R_rot,
                                     uint8_t *mask, int32_t *counts, int32_t *info)
{
    if (!h || B < 1 || B > h->cfg.max_batch) return rpe_invalid(h, "rpe_pair_homographies");
    int rc = homography_check(h, "rpe_pair_homographies", iters, threshold_px);
    if (rc) return rc;
    // d_n1 / d_n2, d_rstate and d_status must still hold the run's (a stage call or a put overwrote them)
    rc = last_run_gate(h, "rpe_pair_homographies", B, NEED_UNCHUNKED | NEED_PER_MATCH | NEED_COUNT | NEED_TABLE);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = homography_alloc(h)) != RPE_OK) return rc;
    return homography_run(h, last_run_first(h, B), iters, threshold_px, true, H, R_rot, mask, counts, info);
}

// ---- pair proposals (rpe_frames_similar / rpe_similarity_hamming; NOT in the reference): similarity scores between frames
// and a top-k candidate selection (the definitions: include/rpe_amd.h; the kernels: similar_kernels.hip).
// The checks the two forms share, host side, in front of any device call.  n_frames: the store's slots or the stage call's
// frames; filled: the store's flags, or null
static int similar_check(rpe_handle *h, const char *who, int n_frames, const uint8_t *filled, int nq, const int32_t *q, int nt, const int32_t *t,
                         int step, int max_distance, int k, const int32_t *scores, const int32_t *cand, const int32_t *cand_score, const int32_t *n_cand)
{
    if (!q || !t || nq < 1 || nt < 1) return rpe_invalid(h, who, "a null list, or nq < 1 or nt < 1");
    if (step < 1) return rpe_invalid(h, who, "step must be >= 1");
    if (max_distance < 0 || max_distance > 256) return rpe_invalid(h, who, "max_distance must be 0 ... 256");
    if (k < 0 || k > RPE_SIMILAR_MAX_K) return rpe_invalid(h, who, "k must be 0 ... RPE_SIMILAR_MAX_K");
    const int trio = (cand != nullptr) + (cand_score != nullptr) + (n_cand != nullptr);
    if (trio != 0 && trio != 3) return rpe_invalid(h, who, "cand, cand_score and n_cand must all be given or all be NULL");
    if (!scores && !trio) return rpe_invalid(h, who, "no output asked for");
    for (int s = 0; s < 2; ++s) {
        const int32_t *l = s ? t : q;
        for (int i = 0, n = s ? nt : nq; i < n; ++i) {
            if (l[i] < 0 || l[i] >= n_frames) return rpe_invalid(h, who, filled ? "slot outside the store" : "frame index outside 0 ... F-1");
            if (filled && !filled[(size_t)l[i]]) return rpe_invalid(h, who, "a list names an empty slot");
        }
    }
    if ((long long)nq * nt > 0x7FFFFFFFLL) { h->err = std::string(who) + ": nq * nt exceeds 2^31 - 1"; return RPE_ERR_CAPACITY; }
    return RPE_OK;
}

// Behind the checks and hipSetDevice: the buffer set, the tables, the launches over the features (desc, count), the fetch
static int similar_run(rpe_handle *h, const uint8_t *desc, const int *count, int nq, const int32_t *q, int nt, const int32_t *t,
                       int step, int max_distance, const int32_t *q_time, const int32_t *t_time, int exclude, int min_score, int k,
                       int32_t *scores, int32_t *cand, int32_t *cand_score, int32_t *n_cand)
{
    const size_t NQ = (size_t)nq, NT = (size_t)nt, ck = cand ? NQ * (size_t)k : 0;
    RpeSimilarBufs &b = h->sim;
    const std::initializer_list<RpeBufPiece> pieces = {
        buf_piece(b.q, NQ, q), buf_piece(b.t, NT, t), buf_piece(b.qtime, q_time ? NQ : 0, q_time), buf_piece(b.ttime, t_time ? NT : 0, t_time),
        buf_piece(b.scores, NQ * NT), buf_piece(b.cand, ck), buf_piece(b.cscore, ck), buf_piece(b.ncand, cand ? NQ : 0)};
    if (int rc = rpe_bufset_fit(h, b.set, pieces)) return rc;
    if (int rc = rpe_bufset_upload(h, pieces)) return rc;
    RpeSimilarJob job;
    job.desc = desc; job.count = count;
    job.nq = nq; job.nt = nt; job.q = b.q; job.t = b.t;
    job.step = std::min(step, std::max(h->lay.kcap, 1));       // a stride of the capacity or more samples descriptor 0 alone
    job.max_distance = max_distance; job.same = nq == nt && memcmp(q, t, sizeof(int32_t) * NQ) == 0;
    job.q_time = q_time ? b.qtime : b.q; job.t_time = t_time ? b.ttime : b.t;      // no times: the slot numbers
    job.exclude = exclude; job.min_score = min_score; job.k = k; job.scores = b.scores;
    // k == 0 selects nothing: every row's count is 0, written below without a launch
    const bool select = cand && k > 0;
    job.cand = select ? b.cand : nullptr; job.cand_score = b.cscore; job.n_cand = b.ncand;
    rpe_launch_similar(h, job);
    HIPCHK(h, hipGetLastError());
    if (cand && !select) memset(n_cand, 0, sizeof(int32_t) * NQ);
    // the wait also covers the uploads: the lists and times have left the caller's arrays
    return fetch(h, {{scores, b.scores, sizeof(int) * NQ * NT}, {select ? cand : nullptr, b.cand, sizeof(int) * ck},
                     {select ? cand_score : nullptr, b.cscore, sizeof(int) * ck}, {select ? n_cand : nullptr, b.ncand, sizeof(int) * NQ}});
}

static int similar_hamming_only(rpe_handle *h, const char *who)
{
    if (h->cfg.feature_method == RPE_FEATURE_SIFT || h->cfg.norm_type != RPE_NORM_HAMMING)
        return rpe_invalid(h, who, "Hamming handles only (ORB with RPE_NORM_HAMMING)");
    return RPE_OK;
}

extern "C" int rpe_frames_similar(rpe_handle *h, int nq, const int32_t *q_slots, int nt, const int32_t *t_slots,
                                  int step, int max_distance, const int32_t *q_time, const int32_t *t_time,
                                  int exclude, int min_score, int k,
                                  int32_t *scores, int32_t *cand, int32_t *cand_score, int32_t *n_cand)
{
    const char *who = "rpe_frames_similar";
    if (!h) return rpe_invalid(h, who);
    if (int rc = similar_hamming_only(h, who)) return rc;
    if (h->fs.cap == 0) return rpe_invalid(h, who, "no frame store (rpe_frames_reserve)");
    if (int rc = similar_check(h, who, h->fs.cap, h->fs.filled.data(), nq, q_slots, nt, t_slots, step, max_distance, k, scores, cand, cand_score, n_cand)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // reads the store, writes sim.set: the last run and what is fetched from it stay as they are
    return similar_run(h, h->fs.d_desc, h->fs.d_count, nq, q_slots, nt, t_slots, step, max_distance, q_time, t_time, exclude, min_score, k,
                       scores, cand, cand_score, n_cand);
}

extern "C" int rpe_similarity_hamming(rpe_handle *h, const uint8_t *h_desc, const int32_t *n, int F,
                                      int nq, const int32_t *q_idx, int nt, const int32_t *t_idx,
                                      int step, int max_distance, const int32_t *q_time, const int32_t *t_time,
                                      int exclude, int min_score, int k,
                                      int32_t *scores, int32_t *cand, int32_t *cand_score, int32_t *n_cand)
{
    const char *who = "rpe_similarity_hamming";
    if (!h || !h_desc || !n || F < 1) return rpe_invalid(h, who);
    if (int rc = similar_hamming_only(h, who)) return rc;
    if (F > h->n_img_cap) { h->err = std::string(who) + ": more than 2*max_batch frames"; return RPE_ERR_CAPACITY; }
    if (int rc = check_desc_counts(h, n, F)) return rc;
    if (int rc = similar_check(h, who, F, nullptr, nq, q_idx, nt, t_idx, step, max_distance, k, scores, cand, cand_score, n_cand)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    last_run_end(h);                            // overwrites the workspace's features
    // frame f on the workspace slot f
    if (int rc = upload(h, {{h->d_desc, h_desc, (size_t)h->lay.kcap * 32 * F}, {h->d_kp_count, n, sizeof(int) * (size_t)F}})) return rc;
    return similar_run(h, h->d_desc, h->d_kp_count, nq, q_idx, nt, t_idx, step, max_distance, q_time, t_time, exclude, min_score, k,
                       scores, cand, cand_score, n_cand);
}

// ---------------------------------------------------------------- the track scene (track_scene.h)
// What rpe_triangulate_tracks and rpe_bundle_windows share.  Phase 1 of its check, in front of the empty-call return: the
// scalars and the CSR shape, then the cameras (K as the one pinhole record it becomes)
static int scene_check_shape(rpe_handle *h, const char *who, const RpeSceneArgs &a)
{
    if (const char *what = rpe_scene_check_shape(a)) return rpe_invalid(h, who, what);
    if (a.K) h->scene.cam_k = rpe_camera{a.K[0], a.K[4], a.K[2], a.K[5], {0., 0., 0., 0., 0., 0., 0., 0.}};
    return a.K ? check_cameras(h, &h->scene.cam_k, 1, who) : check_cameras(h, a.cams, a.n_frames, who);
}
// Behind phase 2 (rpe_scene_check_arrays: n_obs) and hipSetDevice: the scene buffers fitted to this call, the uploads, the device view
static int scene_upload(rpe_handle *h, const RpeSceneArgs &a, size_t n_obs, RpeTrackScene *sc)
{
    RpeSceneBufs &b = h->scene;
    const size_t nt = (size_t)a.n_tracks, nf = (size_t)a.n_frames, nc = a.K ? 1 : nf;
    const std::initializer_list<RpeBufPiece> pieces = {
        buf_piece(b.tstart, nt + 1, a.track_start), buf_piece(b.oframe, n_obs, a.obs_frame), buf_piece(b.oxy, n_obs, a.obs_xy), buf_piece(b.R, 9 * nf, a.R_abs),
        buf_piece(b.T, 3 * nf, a.T_abs), buf_piece(b.cams, nc, a.K ? &b.cam_k : a.cams)};
    if (int rc = rpe_bufset_fit(h, b.set, pieces)) return rc;
    if (int rc = rpe_bufset_upload(h, pieces)) return rc;
    *sc = {a.n_tracks, (int)n_obs, a.K ? 0 : 1, b.tstart, b.oframe, b.oxy, b.R, b.T, b.cams};
    return RPE_OK;
}

// ---------------------------------------------------------------- track points (rpe_triangulate_tracks)
// Every check on the host first, the buffers, the uploads, the two kernels, the fetch.  Neither the workspace nor the record
// of the last run is touched.
extern "C" int rpe_triangulate_tracks(rpe_handle *h, int n_tracks, const int32_t *track_start, const int32_t *obs_frame, const float *obs_xy,
                                      int n_frames, const double *R_abs, const double *T_abs, const int32_t *frame_group, const double *K,
                                      const rpe_camera *cams, double threshold_px, int min_views, double max_cos, int max_iters,
                                      double *points, int32_t *info, double *rms, double *min_cos, uint8_t *obs_flag, double *obs_err)
{
    const char *who = "rpe_triangulate_tracks";
    if (!h) return rpe_invalid(h, who);
    const RpeSceneArgs scene = {n_tracks, track_start, obs_frame, obs_xy, n_frames, R_abs, T_abs, K, cams};
    if (int rc = check_positive(h, who, "threshold_px", threshold_px)) return rc;
    if (min_views < 2) return rpe_invalid(h, who, "min_views must be >= 2");
    if (!(max_cos > -1. && max_cos <= 1.)) return rpe_invalid(h, who, "max_cos must lie in (-1, 1]");
    if (max_iters < 0 || max_iters > 100) return rpe_invalid(h, who, "max_iters must be 0 ... 100");
    if (int rc = scene_check_shape(h, who, scene)) return rc;
    if (n_tracks == 0) return RPE_OK;
    size_t no;
    if (const char *what = rpe_scene_check_arrays(scene, &no)) return rpe_invalid(h, who, what);
    const size_t nt = (size_t)n_tracks, nf = (size_t)n_frames;
    for (size_t f = 0; f < nf; ++f) {
        if (frame_group && frame_group[f] < 0) continue;
        if (!all_finite(R_abs + f * 9, 9) || !all_finite(T_abs + f * 3, 3)) return rpe_invalid(h, who, "a non-finite pose of a frame that has a group");
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t no1 = std::max(no, (size_t)1);
    // the buffers of the call beside the scene: per track, per observation, per frame
    RpeTrackPointBufs &b = h->tp;
    const std::initializer_list<RpeBufPiece> pieces = {
        buf_piece(b.points, 3 * nt), buf_piece(b.info, 4 * nt), buf_piece(b.rms, nt), buf_piece(b.mincos, nt), buf_piece(b.obs, RPE_TRACK_POINT_OBS_BYTES * no1),
        buf_piece(b.oflag, no1), buf_piece(b.oerr, no1), buf_piece(b.group, nf, frame_group)};
    if (int rc = rpe_bufset_fit(h, b.set, pieces)) return rc;
    RpeTrackPointJob job = {{}, min_views, max_iters, threshold_px, max_cos, frame_group ? b.group : nullptr};
    if (int rc = scene_upload(h, scene, no, &job.scene)) return rc;
    if (int rc = rpe_bufset_upload(h, pieces)) return rc;
    rpe_launch_track_points(h, job);
    HIPCHK(h, hipGetLastError());
    // the wait also covers the uploads: the inputs have left the caller's arrays
    return fetch(h, {{points, b.points, sizeof(double) * 3 * nt}, {info, b.info, sizeof(int) * 4 * nt}, {rms, b.rms, sizeof(double) * nt},
                     {min_cos, b.mincos, sizeof(double) * nt}, {obs_flag, b.oflag, no}, {obs_err, b.oerr, sizeof(double) * no}});
}

// ---------------------------------------------------------------- window bundles (rpe_bundle_windows)
// Every check on the host first, the buffers, the uploads, the three kernels, the fetch.  Neither the workspace nor the record
// of the last run is touched.
extern "C" int rpe_bundle_windows(rpe_handle *h, int n_tracks, const int32_t *track_start, const int32_t *obs_frame, const float *obs_xy,
                                  const double *points0, const uint8_t *point_use, const uint8_t *obs_use,
                                  int n_frames, const double *R_abs, const double *T_abs, const double *K, const rpe_camera *cams,
                                  int n_win, const int32_t *win_start, const int32_t *win_frame, int max_points, int min_obs, int max_iters,
                                  double *R_out, double *T_out, double *points, int32_t *point_track, int32_t *counts, int32_t *info,
                                  double *rms)
{
    const char *who = "rpe_bundle_windows";
    if (!h) return rpe_invalid(h, who);
    const RpeSceneArgs scene = {n_tracks, track_start, obs_frame, obs_xy, n_frames, R_abs, T_abs, K, cams};
    if (n_win < 0) return rpe_invalid(h, who, "n_win must be >= 0");
    if (max_points < 1) return rpe_invalid(h, who, "max_points must be >= 1");
    if (max_points > RPE_WINDOW_MAX_POINTS) { h->err = std::string(who) + ": max_points exceeds RPE_WINDOW_MAX_POINTS"; return RPE_ERR_CAPACITY; }
    if (min_obs < 0) return rpe_invalid(h, who, "min_obs must be >= 0");
    if (max_iters < 1 || max_iters > 100) return rpe_invalid(h, who, "max_iters must be 1 ... 100");
    if (int rc = scene_check_shape(h, who, scene)) return rc;
    if (n_win == 0) return RPE_OK;
    if (!win_start || !win_frame || (n_tracks > 0 && !points0)) return rpe_invalid(h, who);
    size_t no;
    if (const char *what = rpe_scene_check_arrays(scene, &no)) return rpe_invalid(h, who, what);
    const size_t nt = (size_t)n_tracks, nw = (size_t)n_win;
    if (win_start[0] != 0) return rpe_invalid(h, who, "win_start[0] must be 0");
    for (int w = 0; w < n_win; ++w) {
        const int W = win_start[w + 1] - win_start[w];
        if (W < 0) return rpe_invalid(h, who, "win_start must not decrease");
        if (W < 2 || W > RPE_WINDOW_MAX_VIEWS) return rpe_invalid(h, who, "a window must have 2 ... RPE_WINDOW_MAX_VIEWS frames");
        const int32_t *f = win_frame + win_start[w];
        for (int p = 0; p < W; ++p) {
            if (f[p] < 0 || f[p] >= n_frames) return rpe_invalid(h, who, "a window frame outside 0 ... n_frames - 1");
            for (int q = 0; q < p; ++q)
                if (f[q] == f[p]) return rpe_invalid(h, who, "a frame repeated inside a window");
            if (!all_finite(R_abs + (size_t)f[p] * 9, 9) || !all_finite(T_abs + (size_t)f[p] * 3, 3))
                return rpe_invalid(h, who, "a non-finite pose of a frame that a window names");
        }
    }
    for (size_t t = 0; t < nt; ++t)
        if ((!point_use || point_use[t]) && !all_finite(points0 + 3 * t, 3)) return rpe_invalid(h, who, "a non-finite start point of a used track");
    const size_t nwf = (size_t)win_start[n_win], slots = nw * (size_t)max_points;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // the buffers of the call beside the scene: per track, per observation, per window frame, per window, per window and point slot
    RpeWindowBufs &b = h->wb;
    const std::initializer_list<RpeBufPiece> pieces = {
        buf_piece(b.points0, 3 * nt, points0), buf_piece(b.puse, nt, point_use), buf_piece(b.obs, RPE_WINDOW_OBS_BYTES * no), buf_piece(b.ouse, no, obs_use),
        buf_piece(b.wstart, nw + 1, win_start), buf_piece(b.wframe, nwf, win_frame), buf_piece(b.Rout, 9 * nwf), buf_piece(b.Tout, 3 * nwf),
        buf_piece(b.counts, 4 * nw), buf_piece(b.info, 4 * nw), buf_piece(b.rms, 2 * nw), buf_piece(b.fcnt, RPE_WINDOW_MAX_VIEWS * nw), buf_piece(b.ptrack, slots),
        buf_piece(b.pobs, RPE_WINDOW_SLOT_OBS * slots), buf_piece(b.state, RPE_WINDOW_STATE_DOUBLES * slots), buf_piece(b.points, 3 * slots)};
    if (int rc = rpe_bufset_fit(h, b.set, pieces)) return rc;
    RpeWindowJob job = {{}, n_win, max_points, min_obs, max_iters, b.points0, point_use ? b.puse : nullptr, obs_use ? b.ouse : nullptr, b.wstart, b.wframe};
    if (int rc = scene_upload(h, scene, no, &job.scene)) return rc;
    if (int rc = rpe_bufset_upload(h, pieces)) return rc;
    rpe_launch_windows(h, job);
    HIPCHK(h, hipGetLastError());
    // the wait also covers the uploads: the inputs have left the caller's arrays
    return fetch(h, {{R_out, b.Rout, sizeof(double) * 9 * nwf}, {T_out, b.Tout, sizeof(double) * 3 * nwf}, {points, b.points, sizeof(double) * 3 * slots},
                     {point_track, b.ptrack, sizeof(int) * slots}, {counts, b.counts, sizeof(int) * 4 * nw}, {info, b.info, sizeof(int) * 4 * nw},
                     {rms, b.rms, sizeof(double) * 2 * nw}});
}

// ---------------------------------------------------------------- pose graphs (rpe_optimise_graphs)
// Every check on the host first, then the active set and the tables of the kernel (graph_plan.h, which the host tests run),
// the buffers, the uploads, the kernel, the fetch.  Neither the workspace nor the record of the last run is touched.
extern "C" int rpe_optimise_graphs(rpe_handle *h, int n_frames, const double *R_abs, const double *T_abs,
                                   int n_graphs, const int32_t *graph_start, const int32_t *graph_frame, const uint8_t *fixed,
                                   const int32_t *edge_start, const int32_t *edge_i, const int32_t *edge_j, const double *edge_R,
                                   const double *edge_t, const double *edge_w, const int32_t *edge_kind,
                                   double huber, int max_iters, int cg_iters, double cg_tol,
                                   double *R_out, double *T_out, int32_t *counts, int32_t *info, double *cost, double *edge_chi,
                                   uint8_t *edge_used)
{
    const char *who = "rpe_optimise_graphs";
    if (!h) return rpe_invalid(h, who);
    const RpeGraphArgs args = {n_frames, R_abs, T_abs, n_graphs, graph_start, graph_frame, fixed, edge_start, edge_i, edge_j,
                               edge_R, edge_t, edge_w, edge_kind, huber, max_iters, cg_iters, cg_tol};
    RpeGraphPlan plan;
    const RpeGraphRefusal no = rpe_graph_check(args, plan);
    if (no.code) { h->err = std::string(who) + ": " + (no.text ? no.text : RPE_NULL_ARGUMENT_TEXT); return no.code; }
    if (n_graphs == 0) return RPE_OK;
    rpe_graph_build(args, plan);
    const size_t ng = (size_t)n_graphs, nf = (size_t)graph_start[n_graphs], ne = (size_t)edge_start[n_graphs];
    const size_t nfr = plan.free_pos.size(), nus = plan.used_edge.size(), nadj = plan.adj.size() / 2, nF = (size_t)n_frames;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    RpeGraphBufs &b = h->pg;
    const std::initializer_list<RpeBufPiece> pieces = {
        buf_piece(b.Rabs, 9 * nF, R_abs), buf_piece(b.Tabs, 3 * nF, T_abs), buf_piece(b.eR, 9 * ne, edge_R), buf_piece(b.et, 3 * ne, edge_t),
        buf_piece(b.ew, 2 * ne, edge_w), buf_piece(b.gstart, ng + 1, graph_start), buf_piece(b.gframe, nf, graph_frame), buf_piece(b.estart, ng + 1, edge_start),
        buf_piece(b.fstart, ng + 1, plan.free_start.data()), buf_piece(b.ustart, ng + 1, plan.used_start.data()), buf_piece(b.precode, ng, plan.precode.data()),
        buf_piece(b.fpos, nfr, plan.free_pos.data()), buf_piece(b.astart, nfr + 1, plan.adj_start.data()), buf_piece(b.uedge, nus, plan.used_edge.data()),
        buf_piece(b.ei, ne, plan.ei.data()), buf_piece(b.ej, ne, plan.ej.data()), buf_piece(b.ekind, ne, edge_kind), buf_piece(b.info, 4 * ng),
        buf_piece(b.adj, nadj, plan.adj.data()), buf_piece(b.Rout, 9 * nf), buf_piece(b.Tout, 3 * nf), buf_piece(b.Rn, 9 * nf), buf_piece(b.Tn, 3 * nf),
        buf_piece(b.eb, RPE_GRAPH_EDGE_DOUBLES * nus), buf_piece(b.fb, RPE_GRAPH_FRAME_DOUBLES * nfr), buf_piece(b.chi, 2 * std::max(ne, (size_t)1)),
        buf_piece(b.cost, 2 * ng)};
    if (int rc = rpe_bufset_fit(h, b.set, pieces)) return rc;
    if (int rc = rpe_bufset_upload(h, pieces)) return rc;
    if (ne > 0) HIPCHK(h, hipMemsetAsync(b.chi, 0, sizeof(double) * 2 * ne, h->stream));
    const RpeGraphJob job = {n_graphs, max_iters, cg_iters, huber, cg_tol, b.Rabs, b.Tabs, b.eR, b.et, b.ew, b.gstart, b.gframe, b.estart,
                             b.fstart, b.ustart, b.precode, b.fpos, b.astart, b.uedge, b.ei, b.ej, b.ekind, b.adj};
    rpe_launch_graphs(h, job);
    HIPCHK(h, hipGetLastError());
    // the wait also covers the uploads: the host tables above and the caller's arrays have been read
    if (int rc = fetch(h, {{R_out, b.Rout, sizeof(double) * 9 * nf}, {T_out, b.Tout, sizeof(double) * 3 * nf}, {info, b.info, sizeof(int) * 4 * ng},
                           {cost, b.cost, sizeof(double) * 2 * ng}, {edge_chi, b.chi, sizeof(double) * 2 * ne}})) return rc;
    if (counts) memcpy(counts, plan.counts.data(), sizeof(int) * 4 * ng);
    if (edge_used && ne > 0) memcpy(edge_used, plan.used.data(), ne);
    return RPE_OK;
}

// ---- the stage forms of the refinement and the homography: stage_begin (rpe_api.hip), then the feature's own buffers and run
static int stage_refine(rpe_handle *h, const char *who, const double *h_R0, const double *h_t0, const float *h_pts1,
                        const float *h_pts2, const uint8_t *h_mask, const int32_t *m, int B, const double *K,
                        const rpe_camera *cam1, const rpe_camera *cam2, int max_iters, double *R, double *t, int32_t *inliers,
                        int32_t *info, double *rms)
{
    RpeRun run;
    int rc = stage_begin(h, who, h_pts1, h_pts2, m, B, K, cam1, cam2, run);
    if (rc) return rc;
    if ((rc = refine_alloc(h)) != RPE_OK) return rc;
    if ((rc = upload(h, {{h->d_mask, h_mask, (size_t)h->cfg.max_matches * B}, {h->ref.R0, h_R0, sizeof(double) * 9 * B},
                         {h->ref.t0, h_t0, sizeof(double) * 3 * B}})) != RPE_OK) return rc;
    return refine_run(h, run, max_iters, false, R, t, inliers, info, rms);
}

extern "C" int rpe_find_homography(rpe_handle *h, const float *h_pts1, const float *h_pts2, const int32_t *m, int B,
                                   const double K[9], int iters, double threshold_px, double *H, double *R_rot, uint8_t *mask,
                                   int32_t *counts, int32_t *info)
{
    if (!h || !h_pts1 || !h_pts2 || !m || !K || B < 1) return rpe_invalid(h, "rpe_find_homography");
    if (int rc = check_batch(h, B)) return rc;
    int rc = homography_check(h, "rpe_find_homography", iters, threshold_px);
    if (rc) return rc;
    if ((rc = check_match_counts(h, m, B)) != RPE_OK) return rc;
    RpeRun run;
    if ((rc = stage_begin(h, "rpe_find_homography", h_pts1, h_pts2, m, B, K, nullptr, nullptr, run)) != RPE_OK) return rc;
    if ((rc = homography_alloc(h)) != RPE_OK) return rc;
    rpe_launch_normalise(h, run);
    return homography_run(h, run, iters, threshold_px, false, H, R_rot, mask, counts, info);
}

extern "C" int rpe_refine_pose_points(rpe_handle *h, const double *h_R0, const double *h_t0, const float *h_pts1,
                                      const float *h_pts2, const uint8_t *h_mask, const int32_t *m, int B, const double K[9],
                                      int max_iters, double *R, double *t, int32_t *inliers, int32_t *info, double *rms)
{
    if (!h || !h_R0 || !h_t0 || !h_pts1 || !h_pts2 || !h_mask || !m || !K || B < 1) return rpe_invalid(h, "rpe_refine_pose_points");
    if (int rc = check_batch(h, B)) return rc;      // in front of max_iters, as ever
    if (max_iters < 1 || max_iters > 100) return rpe_invalid(h, "rpe_refine_pose_points", "max_iters must be 1 ... 100");
    return stage_refine(h, "rpe_refine_pose_points", h_R0, h_t0, h_pts1, h_pts2, h_mask, m, B, K, nullptr, nullptr, max_iters, R, t, inliers, info, rms);
}

extern "C" int rpe_refine_pose_points_cameras(rpe_handle *h, const double *h_R0, const double *h_t0, const float *h_pts1,
                                              const float *h_pts2, const uint8_t *h_mask, const int32_t *m, int B,
                                              const rpe_camera *cam1, const rpe_camera *cam2, int max_iters, double *R, double *t,
                                              int32_t *inliers, int32_t *info, double *rms)
{
    if (!h || !h_R0 || !h_t0 || !h_pts1 || !h_pts2 || !h_mask || !m || !cam1 || !cam2 || B < 1) return rpe_invalid(h, "rpe_refine_pose_points_cameras");
    if (max_iters < 1 || max_iters > 100) return rpe_invalid(h, "rpe_refine_pose_points_cameras", "max_iters must be 1 ... 100");
    return stage_refine(h, "rpe_refine_pose_points_cameras", h_R0, h_t0, h_pts1, h_pts2, h_mask, m, B, nullptr, cam1, cam2, max_iters, R, t, inliers, info, rms);
}
