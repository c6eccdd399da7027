// cloud_nn.hip — exact nearest neighbour of every point of one cloud in ANOTHER cloud (gfx950): the primitive under the
// LiDAR chamfer metric (street_gaussians_ns/data/utils/geometric_metric.py:59-69, open3d's
// compute_point_cloud_distance, two KD-tree sweeps on the CPU in the reference).  For every query row the smallest
// |q - t_j| over all target rows j, and that j; the clouds are unrelated, so nothing is excluded.
//
// Pipeline (all on `stream`, no host synchronisation):
//   knn_build_tree     the tree of knn.hip over the TARGET (knn_tree.h: box, Morton keys, sort, 64-point leaves, AABB heap)
//   knn_morton         the same kernel over the QUERIES with the target's partial boxes: every query is keyed in the
//                      target's Morton cube, coordinates outside it clamped onto its faces
//   sgn_sort_pairs     (key, id) of the queries, so that 64 consecutive queries are neighbours in space
//   cloud_nn_query     one wave per 64 sorted queries.  Seed leaf: the target leaf whose key range holds the key of the
//                      wave's middle query (a wave-uniform binary search over the leaves' first keys, which the build left
//                      in the workspace).  The seed leaf is scanned first; then the walk of knn_query with "own leaf"
//                      replaced by "seed leaf": a wave-uniform stack in LDS, the half nearer the seed popped first, a node
//                      entered only if ballot(valid && box_d2 < best_d2) is non-zero, a leaf's 64 candidates read with
//                      wave-uniform (scalar) loads and tested by every lane against one register best.
//
//   cloud_nn_query_sparse   the form for FEW queries against a large target (n_query * 16 <= n_target).  Sixty-four
//                      sorted queries then lie ~64 * 16 target leaves apart along the curve, and a wave that walks for
//                      all of them together visits the union of 64 unrelated walks (63 uniform queries against 10 037
//                      points: 150 of the 157 leaves, for every lane).  Here one wave takes ONE query, held in scalar
//                      registers: the same seed search on the query's own key (no query sort), the same walk, and a leaf
//                      is scanned with one candidate per LANE (a coalesced 1 KiB load), a wave minimum, and the lowest
//                      lane among equal minima (the first in leaf order) replacing the best only if strictly nearer.
//                      The switch point is an estimate, not a timing: at r target leaves per query a shared walk
//                      scans ~r + 20 leaves per wave for all 64 lanes, a single walk ~6 leaves per query with one
//                      dependent load and a wave reduction each.
//
// Exactness and determinism are those of knn.hip: fp32 direct differences without FMA, a box distance with the same
// operation order (box_d2 <= d2 bit for bit for every point of the box, so the strict pruning test never drops a candidate
// the strict insertion test would keep), the first of equal distances in visit order kept, and a visit order that is a
// function of the two sorted inputs alone.  The seed only decides how soon `best` becomes tight, never the result's
// distance.  The only atomic is the optional `visited` sum.
#include "knn_tree.h"

#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "cloud_nn.hip is written for gfx950 (MI355X) only"
#endif

namespace {

struct CloudLayout {
    KnnLayout T;           // the target's tree
    int64_t *qkeys_in, *qkeys_out;
    int32_t *qids_in, *qids_out;
    void *qsort_ws;
    size_t qsort_ws_bytes, total;
};

CloudLayout cloud_layout(int n_target, int n_query, void *ws) {
    CloudLayout C{};
    C.T = knn_layout(n_target, ws);
    char *base = (char *)ws;
    size_t off = C.T.total;
    auto take = [&](size_t b) { char *q = base ? base + off : nullptr; off += knn_align(b); return q; };
    C.qkeys_in = (int64_t *)take((size_t)n_query * 8);
    C.qkeys_out = (int64_t *)take((size_t)n_query * 8);
    C.qids_in = (int32_t *)take((size_t)n_query * 4);
    C.qids_out = (int32_t *)take((size_t)n_query * 4);
    C.qsort_ws_bytes = sgn_sort_workspace_bytes(n_query);
    C.qsort_ws = (void *)take(C.qsort_ws_bytes);
    C.total = off;
    return C;
}

// all 64 candidates of target leaf `leaf` against this lane's query; wave-uniform addresses -> scalar loads
__device__ __forceinline__ void cloud_nn_scan_leaf(const float4 *__restrict__ pts, int leaf, float qx, float qy, float qz,
                                                   float &best_d2, int &best_j) {
    const int base = leaf * KNN_LEAF;
    const float4 *c = pts + base;
#pragma unroll 4
    for (int t = 0; t < KNN_LEAF; ++t) {
        const float4 p = c[t];
        const float d2 = knn_d2(qx, qy, qz, p.x, p.y, p.z);
        const bool nearer = d2 < best_d2;          // strict: the first of equal distances stays; a +inf pad never enters
        best_d2 = nearer ? d2 : best_d2;
        best_j = nearer ? base + t : best_j;
    }
}

__global__ __launch_bounds__(64 * KNN_QUERY_WAVES) void cloud_nn_query(
    int n_query, int groups, int leaves, int p2, const float4 *__restrict__ pts, const float4 *__restrict__ nodes,
    const int64_t *__restrict__ tkeys, const int32_t *__restrict__ tids, const float *__restrict__ query,
    const int64_t *__restrict__ qkeys, const int32_t *__restrict__ qids, float *__restrict__ dist,
    int32_t *__restrict__ idx, unsigned long long *__restrict__ visited) {
    __shared__ int stack_lds[KNN_QUERY_WAVES][KNN_STACK];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = __builtin_amdgcn_readfirstlane(blockIdx.x * KNN_QUERY_WAVES + w);
    if (g >= groups) return;
    int *stack = stack_lds[w];
    const int self = g * KNN_LEAF + lane;
    const bool valid = self < n_query;
    const int row = qids[valid ? self : n_query - 1];           // (lanes past the end repeat the last query, masked out)
    const float qx = query[(size_t)row * 3], qy = query[(size_t)row * 3 + 1], qz = query[(size_t)row * 3 + 2];

    // seed: the last target leaf whose first key is <= the wave's middle key (leaf 0 if there is none); leaves' first
    // keys ascend, and (leaves - 1) * 64 < n_target keeps every probe inside the sorted keys
    const int probe = g * KNN_LEAF + KNN_LEAF / 2;
    const int64_t key = qkeys[probe < n_query ? probe : n_query - 1];
    int lo = 1, hi = leaves;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tkeys[(size_t)mid * KNN_LEAF] <= key) lo = mid + 1; else hi = mid;
    }
    const int seed = lo - 1;

    float best_d2 = INFINITY;
    int best_j = -1;
    const unsigned long long nvalid = __popcll(__ballot(valid));
    unsigned long long nleaf = 1;
    cloud_nn_scan_leaf(pts, seed, qx, qy, qz, best_d2, best_j);

    const int own = p2 + seed;
    int sp = 0;
    if (own != 1) {                       // (a tree of one leaf: nothing else to visit)
        stack[0] = 1;
        sp = 1;
    }
    while (sp > 0) {
        --sp;
        const int v = __builtin_amdgcn_readfirstlane(stack[sp]);
        const float4 blo = nodes[(size_t)v * 2], bhi = nodes[(size_t)v * 2 + 1];
        const float bd2 = knn_box_d2(qx, qy, qz, blo, bhi);
        if (__ballot(valid && bd2 < best_d2) == 0) continue;
        if (v >= p2) {
            if (v - p2 >= leaves) continue;      // an empty leaf of the padding: only a non-finite query gets here
            cloud_nn_scan_leaf(pts, v - p2, qx, qy, qz, best_d2, best_j);
            ++nleaf;
            continue;
        }
        // as knn_query: children of v cover leaves [.., mid) and [mid, ..); the half holding (or nearer in Morton order
        // to) the seed leaf is popped first, the seed leaf itself is never pushed; <= levels + 1 < KNN_STACK entries
        const int lvl = 31 - __builtin_clz(v);
        const int span = p2 >> (lvl + 1);
        const int mid = (v << (31 - __builtin_clz(p2) - lvl)) - p2 + span;
        const int cl = 2 * v, cr = 2 * v + 1;
        const int first = seed < mid ? cl : cr, second = seed < mid ? cr : cl;
        if (second != own) stack[sp++] = second;
        if (first != own) stack[sp++] = first;
    }

    if (visited && lane == 0) atomicAdd(visited, nleaf * KNN_LEAF * nvalid);
    if (!valid) return;
    dist[row] = sqrtf(best_d2);
    if (idx) idx[row] = best_j >= 0 ? tids[best_j] : -1;       // (-1 only for non-finite input)
}

constexpr int CLOUD_SPARSE_RATIO = 16;   // n_query * 16 <= n_target: one wave per query (cloud_nn_query_sparse)

__device__ __forceinline__ float cloud_nn_uniform(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// one wave per query; everything but the candidate in a lane is wave-uniform
__global__ __launch_bounds__(64 * KNN_QUERY_WAVES) void cloud_nn_query_sparse(
    int n_query, int leaves, int p2, const float4 *__restrict__ pts, const float4 *__restrict__ nodes,
    const int64_t *__restrict__ tkeys, const int32_t *__restrict__ tids, const float *__restrict__ query,
    const int64_t *__restrict__ qkeys, float *__restrict__ dist, int32_t *__restrict__ idx,
    unsigned long long *__restrict__ visited) {
    __shared__ int stack_lds[KNN_QUERY_WAVES][KNN_STACK];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = __builtin_amdgcn_readfirstlane(blockIdx.x * KNN_QUERY_WAVES + w);
    if (row >= n_query) return;
    int *stack = stack_lds[w];
    const float qx = query[(size_t)row * 3], qy = query[(size_t)row * 3 + 1], qz = query[(size_t)row * 3 + 2];

    const int64_t key = qkeys[row];              // (unsorted: this form needs no query order)
    int lo = 1, hi = leaves;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tkeys[(size_t)mid * KNN_LEAF] <= key) lo = mid + 1; else hi = mid;
    }
    const int seed = lo - 1;

    float best_d2 = INFINITY;
    int best_j = -1;
    unsigned long long nleaf = 0;
    auto scan = [&](int leaf) {
        const float4 p = pts[(size_t)leaf * KNN_LEAF + lane];
        const float d2 = knn_d2(qx, qy, qz, p.x, p.y, p.z);
        const float m = cloud_nn_uniform(wave_min(d2));
        if (m < best_d2) {                       // strict; among equal minima the lowest lane, the first in leaf order
            best_d2 = m;
            best_j = leaf * KNN_LEAF + __builtin_ctzll(__ballot(d2 == m));
        }
        ++nleaf;
    };
    scan(seed);

    const int own = p2 + seed;
    int sp = 0;
    if (own != 1) {
        stack[0] = 1;
        sp = 1;
    }
    while (sp > 0) {
        --sp;
        const int v = __builtin_amdgcn_readfirstlane(stack[sp]);
        const float4 blo = nodes[(size_t)v * 2], bhi = nodes[(size_t)v * 2 + 1];
        const float bd2 = cloud_nn_uniform(knn_box_d2(qx, qy, qz, blo, bhi));
        if (!(bd2 < best_d2)) continue;
        if (v >= p2) {
            if (v - p2 < leaves) scan(v - p2);   // (an empty leaf of the padding: only a non-finite query gets there)
            continue;
        }
        const int lvl = 31 - __builtin_clz(v);
        const int span = p2 >> (lvl + 1);
        const int mid = (v << (31 - __builtin_clz(p2) - lvl)) - p2 + span;
        const int cl = 2 * v, cr = 2 * v + 1;
        const int first = seed < mid ? cl : cr, second = seed < mid ? cr : cl;
        if (second != own) stack[sp++] = second;
        if (first != own) stack[sp++] = first;
    }

    if (lane != 0) return;
    if (visited) atomicAdd(visited, nleaf * KNN_LEAF);
    dist[row] = sqrtf(best_d2);
    if (idx) idx[row] = best_j >= 0 ? tids[best_j] : -1;
}

}  // namespace

SGN_EXPORT size_t sgn_cloud_nn_workspace_bytes(int n_target, int n_query) {
    if (n_target <= 0 || n_target > KNN_MAX_N || n_query <= 0 || n_query > KNN_MAX_N) return 0;
    return cloud_layout(n_target, n_query, nullptr).total;
}

SGN_EXPORT int sgn_cloud_nn(int n_target, const float *target, int n_query, const float *query, float *dist,
                            int32_t *idx, int64_t *visited, void *ws, size_t ws_bytes, sgn_stream_t stream) {
    SGN_ARG_CHECK(n_target >= 1 && n_target <= KNN_MAX_N, -1);
    SGN_ARG_CHECK(n_query >= 1 && n_query <= KNN_MAX_N, -2);
    SGN_ARG_CHECK(target && query && dist && ws, -3);
    SGN_ARG_CHECK(ws_bytes >= sgn_cloud_nn_workspace_bytes(n_target, n_query), -4);
    hipStream_t s = (hipStream_t)stream;
    const CloudLayout C = cloud_layout(n_target, n_query, ws);
    const int leaves = knn_leaves(n_target), p2 = knn_pow2(leaves), groups = knn_leaves(n_query);
    int nparts = 0;
    int rc = knn_build_tree(n_target, target, C.T, &nparts, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(knn_morton, dim3(sgn_cdiv(n_query, 256)), dim3(256), 0, s, n_query, nparts, query, C.T.partial,
                       C.qkeys_in, C.qids_in);
    SGN_LAUNCH_CHECK();
    if ((int64_t)n_query * CLOUD_SPARSE_RATIO <= (int64_t)n_target) {
        hipLaunchKernelGGL(cloud_nn_query_sparse, dim3(sgn_cdiv(n_query, KNN_QUERY_WAVES)), dim3(64 * KNN_QUERY_WAVES), 0,
                           s, n_query, leaves, p2, C.T.pts, C.T.nodes, C.T.keys_out, C.T.ids_out, query, C.qkeys_in, dist,
                           idx, (unsigned long long *)visited);
        SGN_LAUNCH_CHECK();
        return 0;
    }
    rc = sgn_sort_pairs(n_query, 0, 63, C.qkeys_in, C.qids_in, C.qkeys_out, C.qids_out, C.qsort_ws, C.qsort_ws_bytes,
                        /*documented ballot ranking*/ 0, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(cloud_nn_query, dim3(sgn_cdiv(groups, KNN_QUERY_WAVES)), dim3(64 * KNN_QUERY_WAVES), 0, s,
                       n_query, groups, leaves, p2, C.T.pts, C.T.nodes, C.T.keys_out, C.T.ids_out, query, C.qkeys_out,
                       C.qids_out, dist, idx, (unsigned long long *)visited);
    SGN_LAUNCH_CHECK();
    return 0;
}
