// track_kernels.hip -- multi-view tracks (include/rpe_amd.h, "multi-view tracks"): the connected components of a run's
// match graph by a lock-free union-find, the one-keypoint-per-frame filter, and the CSR observation lists.  Integers
// only; every atomic is a min, an add or a compare-and-swap towards the smaller id, so no result depends on their order.
//
// One launch sequence on the handle's stream (kernel boundaries order the phases):
//   init      parent[id] = id, first-edge word = none, sizes / cursors / conflict flags / counters cleared
//   hook      one thread per match slot: the edge predicate, the per-match edge flag, atomicMin of (edge id * 2 + side) into
//             both nodes' first-edge words, and the union of the two nodes
//   flatten   one thread per node with an edge: label = its root, atomicAdd of the component's size at the root (counted
//             until it exceeds n_frames: beyond that only "more nodes than frames" is read)
//   scan 0    exclusive sum over the nodes of (root of a component of 2 .. n_frames nodes ? size : 0): the start of the
//             component's segment in the member scratch.  A component with more nodes than there are frames conflicts by
//             pigeonhole and is marked without being looked at; one node alone is never a track (min_len >= 2)
//   gather    every node of such a component takes a place in its segment by an atomic cursor (the order inside a segment
//             is arbitrary and used by rank only)
//   rank      one thread per member: streams over its component's segment, counts the members with a smaller id (the
//             observation's rank) and raises the conflict flag when another member has its frame.  Neighbouring threads
//             hold members of the same component and read the same words, so short components pack 64 to a wave.
//   scan 1    exclusive sums over the nodes of (kept root ? 1 : 0) and (kept root ? size : 0): track index and track_start
//   emit      every node of a kept component writes its observation at track_start + rank; the roots count the dropped ones
//   match     match_track of every match slot from its component's root
//   finish    frames seen, the closing entry of track_start
#include "rpe_internal.h"

struct TkArgs {
    RpeTrackJob job;
    int mm, KC, N;                 // max_matches, keypoint capacity, nodes = n_frames * KC
    int *parent, *first, *size, *label, *segstart, *cursor, *rank, *tidx, *tstart, *conflict, *members;   // [N] each
    int *frame_seen;               // [n_frames]
    int2 *partial;                 // [blocks of the scans]
    uint8_t *eflag;                // [P * mm] the match is an edge
    int *mtrack;                   // [P * mm]
    int *counts;                   // [8]: the six of the header, [6] = members gathered (the total of scan 0)
    int *o_tstart, *o_frame, *o_kp;
    float2 *o_xy;
};

constexpr int TK_NONE = 0x7FFFFFFF;      // first-edge word of a node without an edge
constexpr int TK_SCAN_ITEMS = 2048;      // nodes per workgroup of the scans: 8 rounds of 256

__global__ __launch_bounds__(256) void tk_init_kernel(const TkArgs a)
{
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;      // 64-bit: the bound holds for every N an int can be
    if (id < a.N) { a.parent[id] = (int)id; a.first[id] = TK_NONE; a.size[id] = 0; a.cursor[id] = 0; a.conflict[id] = 0; }
    if (id < a.job.n_frames) a.frame_seen[id] = 0;
    if (id < 8) a.counts[id] = 0;
}

// parent words inside the hook kernel: other workgroups lower them while this one reads, so every read is an agent-scope
// load (served from L2, never from this CU's L1) and every write an atomic
__device__ __forceinline__ int tk_parent(const int *parent, int x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x with path halving.  parent[x] <= x always, and a word only ever decreases, so the walk ends
__device__ __forceinline__ int tk_find(int *parent, int x)
{
    for (;;) {
        const int p = tk_parent(parent, x);
        if (p == x) return x;
        const int g = tk_parent(parent, p);
        if (g != p) atomicCAS(parent + x, p, g);       // lost to another writer: that one lowered it too
        x = g;
    }
}

__global__ __launch_bounds__(256) void tk_hook_kernel(const TkArgs a)
{
    const RpeTrackJob &j = a.job;
    const long long total = (long long)j.P * a.mm;
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    bool e = false;
    int na = 0, nb = 0;
    if (o < total) {
        const int p = (int)(o / a.mm), i = (int)(o - (long long)p * a.mm);
        e = (!j.use_pair || j.use_pair[p] != 0) && i < min(j.m_n[p], a.mm);
        if (e && j.rule != RPE_TRACK_EDGES_ALL) {
            e = j.status[p] == RPE_PAIR_OK && j.rmask[o] != 0;
            if (e && j.rule == RPE_TRACK_EDGES_USABLE) e = j.pmask[o] != 0;
        }
        if (e && j.edge) e = j.edge[o] != 0;
        if (e) {
            const int2 f = j.frames[p];
            const int q = j.q[o], t = j.t[o];
            e = (unsigned)q < (unsigned)a.KC && (unsigned)t < (unsigned)a.KC;      // the node arrays' bound
            na = f.x * a.KC + q; nb = f.y * a.KC + t;
        }
        a.eflag[o] = (uint8_t)e;
    }
    const unsigned long long edges = __ballot(e);
    if ((threadIdx.x & 63) == 0 && edges) atomicAdd(a.counts + 2, __popcll(edges));
    if (!e) return;
    atomicMin(a.first + na, (int)(o * 2));
    atomicMin(a.first + nb, (int)(o * 2 + 1));
    // union: the larger root goes under the smaller, so the root of a component ends as its smallest node id whatever
    // the interleaving
    int x = na, y = nb;
    for (;;) {
        x = tk_find(a.parent, x); y = tk_find(a.parent, y);
        if (x == y) break;
        const int hi = max(x, y), lo = min(x, y);
        if (atomicCAS(a.parent + hi, hi, lo) == hi) break;
    }
}

__global__ __launch_bounds__(256) void tk_flatten_kernel(const TkArgs a)
{
    const int id = tk_thread_index(a.N);
    if (id < 0) return;
    int r = -1;
    if (a.first[id] != TK_NONE) {
        r = tk_find(a.parent, id);      // halves the paths the other nodes of the component still have to walk
        // A component with more nodes than the run has frames conflicts whatever its exact size, and that size is no
        // output: counting stops there, or the nodes of a giant component (every match an edge: one wrong match in a
        // hundred joins most of the graph) would queue on one word
        if (tk_parent(a.size, r) <= a.job.n_frames) atomicAdd(a.size + r, 1);
    }
    a.label[id] = r;
}

__device__ __forceinline__ bool tk_kept(const TkArgs &a, int r)
{
    return a.conflict[r] == 0 && a.size[r] >= a.job.min_len;
}

// what node id adds to the two sums of scan MODE
template <int MODE>
__device__ __forceinline__ int2 tk_value(const TkArgs &a, int id)
{
    if (id >= a.N || a.label[id] != id) return make_int2(0, 0);
    const int s = a.size[id];
    if (MODE == 0) return make_int2(s >= 2 && s <= a.job.n_frames ? s : 0, 0);
    return tk_kept(a, id) ? make_int2(1, s) : make_int2(0, 0);
}

template <int MODE>
__global__ __launch_bounds__(256) void tk_scan_reduce_kernel(const TkArgs a)
{
    __shared__ int s_cnt[4];
    int2 v = make_int2(0, 0);
    for (int it = 0; it < TK_SCAN_ITEMS / 256; ++it) {
        const long long id = (long long)blockIdx.x * TK_SCAN_ITEMS + it * 256 + threadIdx.x;
        if (id < a.N) { const int2 w = tk_value<MODE>(a, (int)id); v.x += w.x; v.y += w.y; }
    }
    const int x = block_count(v.x, s_cnt);
    __syncthreads();
    const int y = block_count(v.y, s_cnt);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = make_int2(x, y);
}

// the workgroup sums -> their exclusive prefixes, in place; the totals to tot_x / tot_y.  One workgroup
__global__ __launch_bounds__(256) void tk_scan_partials_kernel(int2 *__restrict__ partial, int nb, int *__restrict__ tot_x, int *__restrict__ tot_y)
{
    __shared__ int s_wave[4];
    int cx = 0, cy = 0;
    for (int base = 0; base < nb; base += 256) {
        const int i = base + threadIdx.x;
        const int2 v = i < nb ? partial[i] : make_int2(0, 0);
        int tx, ty;
        const int ex = block_excl_scan(v.x, s_wave, tx);
        const int ey = block_excl_scan(v.y, s_wave, ty);
        if (i < nb) partial[i] = make_int2(cx + ex, cy + ey);
        cx += tx; cy += ty;
    }
    if (threadIdx.x == 0) { *tot_x = cx; *tot_y = cy; }
}

template <int MODE>
__global__ __launch_bounds__(256) void tk_scan_apply_kernel(const TkArgs a)
{
    __shared__ int s_wave[4];
    int2 carry = a.partial[blockIdx.x];
    for (int it = 0; it < TK_SCAN_ITEMS / 256; ++it) {
        const long long id = (long long)blockIdx.x * TK_SCAN_ITEMS + it * 256 + threadIdx.x;
        const int2 v = id < a.N ? tk_value<MODE>(a, (int)id) : make_int2(0, 0);
        int tx, ty = 0;
        const int ex = block_excl_scan(v.x, s_wave, tx);
        if (MODE == 0) {
            if (id < a.N) a.segstart[id] = carry.x + ex;
        } else {
            const int ey = block_excl_scan(v.y, s_wave, ty);
            if (id < a.N) { a.tidx[id] = carry.x + ex; a.tstart[id] = carry.y + ey; }
        }
        carry.x += tx; carry.y += ty;
    }
}

__global__ __launch_bounds__(256) void tk_gather_kernel(const TkArgs a)
{
    const int id = tk_thread_index(a.N);
    if (id < 0) return;
    const int r = a.label[id];
    if (r < 0) return;
    const int s = a.size[r];
    if (s > a.job.n_frames) { if (id == r) a.conflict[r] = 1; return; }      // pigeonhole
    if (s < 2) return;
    a.members[a.segstart[r] + atomicAdd(a.cursor + r, 1)] = id;              // < segstart[r] + s: every member comes once
}

__global__ __launch_bounds__(256) void tk_rank_kernel(const TkArgs a)
{
    const int j = tk_thread_index(a.counts[6]);
    if (j < 0) return;
    const int x = a.members[j], r = a.label[x];
    const int s = a.size[r], base = a.segstart[r];
    const int lo = x / a.KC * a.KC, hi = lo + a.KC;          // the ids of x's frame
    int rank = 0;
    bool clash = false;
    for (int k = 0; k < s; ++k) {
        const int y = a.members[base + k];
        rank += y < x;
        clash = clash || (y != x && y >= lo && y < hi);
    }
    a.rank[x] = rank;
    if (clash) a.conflict[r] = 1;
}

__global__ __launch_bounds__(256) void tk_emit_kernel(const TkArgs a)
{
    const int id = tk_thread_index(a.N);
    if (id < 0) return;
    const int r = a.label[id];
    if (r < 0) return;
    const bool clash = a.conflict[r] != 0, kept = tk_kept(a, r);
    if (id == r) {
        if (kept) a.o_tstart[a.tidx[r]] = a.tstart[r];
        else atomicAdd(a.counts + (clash ? 3 : 4), 1);
    }
    if (!kept) return;
    const int pos = a.tstart[r] + a.rank[id], f = id / a.KC;
    a.o_frame[pos] = f;
    a.o_kp[pos] = id - f * a.KC;
    const int key = a.first[id];
    float2 xy = make_float2(0.f, 0.f);
    if (a.job.pts1) xy = (key & 1) ? a.job.pts2[key >> 1] : a.job.pts1[key >> 1];
    a.o_xy[pos] = xy;
    a.frame_seen[f] = 1;
}

__global__ __launch_bounds__(256) void tk_match_kernel(const TkArgs a)
{
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= (long long)a.job.P * a.mm) return;
    int v = -1;
    if (a.eflag[o]) {
        const int r = a.label[a.job.frames[o / a.mm].x * a.KC + a.job.q[o]];
        if (tk_kept(a, r)) v = a.tidx[r];
    }
    a.mtrack[o] = v;
}

__global__ __launch_bounds__(256) void tk_finish_kernel(const TkArgs a)
{
    __shared__ int s_cnt[4];
    int n = 0;
    for (int f = threadIdx.x; f < a.job.n_frames; f += 256) n += a.frame_seen[f];
    n = block_count(n, s_cnt);
    if (threadIdx.x == 0) { a.counts[5] = n; a.o_tstart[a.counts[0]] = a.counts[1]; }
}

// The whole sequence for one job.  The buffers are the caller's business (rpe_features.hip, tracks_alloc): the node block holds
// RPE_TRACK_NODE_WORDS arrays of N words
void rpe_launch_tracks(rpe_handle *h, const RpeTrackJob &job)
{
    TkArgs a{};
    a.job = job; a.mm = h->cfg.max_matches; a.KC = h->lay.kcap; a.N = job.n_frames * a.KC;
    int *w = h->tk.node;
    int **arr[RPE_TRACK_NODE_WORDS] = {&a.parent, &a.first, &a.size, &a.label, &a.segstart, &a.cursor, &a.rank, &a.tidx, &a.tstart, &a.conflict, &a.members};
    for (int k = 0; k < RPE_TRACK_NODE_WORDS; ++k) *arr[k] = w + (size_t)k * a.N;
    a.frame_seen = h->tk.seen; a.partial = h->tk.partial; a.eflag = h->tk.eflag; a.mtrack = h->tk.mtrack; a.counts = h->tk.counts;
    a.o_tstart = h->tk.tstart; a.o_frame = h->tk.oframe; a.o_kp = h->tk.okp; a.o_xy = h->tk.oxy;
    const hipStream_t s = h->stream;
    const long long slots = (long long)job.P * a.mm;
    const dim3 blk(256), gn((unsigned)(((long long)std::max(a.N, 8) + 255) / 256)), gm((unsigned)((slots + 255) / 256));
    const int nb = rpe_track_scan_blocks(a.N);
    hipLaunchKernelGGL(tk_init_kernel, gn, blk, 0, s, a);
    hipLaunchKernelGGL(tk_hook_kernel, gm, blk, 0, s, a);
    hipLaunchKernelGGL(tk_flatten_kernel, gn, blk, 0, s, a);
    hipLaunchKernelGGL(tk_scan_reduce_kernel<0>, dim3(nb), blk, 0, s, a);
    hipLaunchKernelGGL(tk_scan_partials_kernel, dim3(1), blk, 0, s, a.partial, nb, a.counts + 6, a.counts + 7);
    hipLaunchKernelGGL(tk_scan_apply_kernel<0>, dim3(nb), blk, 0, s, a);
    hipLaunchKernelGGL(tk_gather_kernel, gn, blk, 0, s, a);
    hipLaunchKernelGGL(tk_rank_kernel, gn, blk, 0, s, a);
    hipLaunchKernelGGL(tk_scan_reduce_kernel<1>, dim3(nb), blk, 0, s, a);
    hipLaunchKernelGGL(tk_scan_partials_kernel, dim3(1), blk, 0, s, a.partial, nb, a.counts + 0, a.counts + 1);
    hipLaunchKernelGGL(tk_scan_apply_kernel<1>, dim3(nb), blk, 0, s, a);
    hipLaunchKernelGGL(tk_emit_kernel, gn, blk, 0, s, a);
    hipLaunchKernelGGL(tk_match_kernel, gm, blk, 0, s, a);
    hipLaunchKernelGGL(tk_finish_kernel, dim3(1), blk, 0, s, a);
}
