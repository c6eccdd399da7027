// knn.hip — exact k-nearest-neighbour search over 3-D points (gfx950), for the initial Gaussian scales.
//
// Replaces sklearn's NearestNeighbors(k+1).kneighbors(x)[:, 1:] as the reference uses it in
// SplatfactoModel.populate_modules (street_gaussians_ns/sgn_splatfacto.py:260-264, k_nearest_sklearn :439-457):
// for every point the k smallest |x_i - x_j| over j != i, ascending, with their j.
//
// Pipeline (all on `stream`, no host synchronisation):
//   knn_bbox_partial   per-block AABB of the points                      -> partial[KNN_BBOX_BLOCKS]
//   knn_morton         every block folds the partial boxes, then one 63-bit Morton key per point (21 bits per axis
//                      over the cube of the largest extent: with 10 bits a far outlier collapses the dense core)
//   sgn_sort_pairs     (key, id) over bits [0, 63), stable, documented ballot ranking (radix_sort.hip)
//   knn_gather         sorted points as float4, padded to whole 64-point leaves with +inf points
//   knn_leaf_box       one wave per leaf: the AABB of its valid points (empty leaves of the power-of-two padding: an
//                      empty box, +inf lower / -inf upper corner, whose distance to anything is +inf)
//   knn_level_box      one launch per tree level: implicit heap (root 1, leaves at P + l), parent = union of children
//   knn_query<K>       one wave per leaf of 64 queries: own leaf first, then a depth-first walk with a wave-uniform
//                      stack in LDS, entering a node only if ballot(box_d2 < kth_d2) is non-zero; a leaf's 64 candidates
//                      are read with wave-uniform (scalar) loads and tested against every lane.
//
// Exactness.  Distances are fp32 direct differences, d2 = (dx*dx + dy*dy) + dz*dz (no FMA: -ffp-contract=off), and a
// box's distance is formed the same way from the per-axis gaps, which are fp-monotone in the point: for every point p
// inside a box B, box_d2(q, B) <= d2(q, p) holds bit for bit, so pruning on `box_d2 < kth_d2` never drops a candidate
// that the insertion test `d2 < kth_d2` would have kept.  The kept set is therefore k smallest fp32 d2 over j != i.
// Both tests are strict: a node or candidate that only ties the current k-th distance is skipped, which bounds the work
// on duplicates and lattices (all points identical: the own leaf alone, 64 candidates per query).
//
// Determinism.  The traversal order is a function of the sorted input alone and the top-k insertion keeps the first
// of equal distances in visit order, so results are bit-identical run to run; the only atomic is the optional
// `visited` counter (a sum).
//
// Top-k: K slots in registers with K a compile-time bucket (1, 2, 4, 8, 16).  For k < K the first K - k slots are
// sentinels at d2 = -1 that no candidate displaces, so the k-th distance is always slot K - 1 and every index into the
// arrays is static (ScratchSize 0).
#include "knn_tree.h"

#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "knn.hip is written for gfx950 (MI355X) only"
#endif

namespace {

template <int K>
struct TopK {
    float d[K];
    int j[K];
    // strict: a candidate equal to a kept distance goes behind it (the first of equal distances stays first).  Every
    // slot is computed from the old values only: shift down from the slot above, take the candidate, or keep.
    __device__ __forceinline__ void insert(float cd, int cj) {
#pragma unroll
        for (int s = K - 1; s > 0; --s) {
            const bool shift = cd < d[s - 1], here = cd < d[s];
            d[s] = shift ? d[s - 1] : here ? cd : d[s];
            j[s] = shift ? j[s - 1] : here ? cj : j[s];
        }
        const bool first = cd < d[0];
        d[0] = first ? cd : d[0];
        j[0] = first ? cj : j[0];
    }
};

// all 64 candidates of leaf `leaf` against this lane's query (sorted index self); wave-uniform addresses -> scalar loads
template <int K>
__device__ __forceinline__ void knn_scan_leaf(const float4 *__restrict__ pts, int leaf, float qx, float qy, float qz,
                                              int self, TopK<K> &top) {
    const int base = leaf * KNN_LEAF;
    const float4 *c = pts + base;
#pragma unroll 4
    for (int t = 0; t < KNN_LEAF; ++t) {
        const float4 p = c[t];
        const float d2 = knn_d2(qx, qy, qz, p.x, p.y, p.z);
        if (d2 < top.d[K - 1] && base + t != self) top.insert(d2, base + t);
    }
}

template <int K>
__global__ __launch_bounds__(64 * KNN_QUERY_WAVES) void knn_query(int n, int k, int leaves, int p2,
                                                                  const float4 *__restrict__ pts,
                                                                  const float4 *__restrict__ nodes,
                                                                  const int32_t *__restrict__ ids,
                                                                  float *__restrict__ dist, int32_t *__restrict__ idx,
                                                                  unsigned long long *__restrict__ visited) {
    __shared__ int stack_lds[KNN_QUERY_WAVES][KNN_STACK];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int leaf = __builtin_amdgcn_readfirstlane(blockIdx.x * KNN_QUERY_WAVES + w);
    if (leaf >= leaves) return;
    int *stack = stack_lds[w];
    const int self = leaf * KNN_LEAF + lane;
    const bool valid = self < n;
    const float4 q = pts[self];
    TopK<K> top;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        top.d[s] = s < K - k ? -1.f : INFINITY;   // sentinels below every real distance: the k-th is slot K - 1
        top.j[s] = -1;
    }
    const unsigned long long nvalid = __popcll(__ballot(valid));
    unsigned long long nleaf = 1;
    knn_scan_leaf<K>(pts, leaf, q.x, q.y, q.z, self, top);

    const int own = p2 + leaf;
    int sp = 0;
    if (own != 1) {                       // (a tree of one leaf: nothing else to visit)
        stack[0] = 1;
        sp = 1;
    }
    while (sp > 0) {
        --sp;
        const int v = __builtin_amdgcn_readfirstlane(stack[sp]);
        const float4 lo = nodes[(size_t)v * 2], hi = nodes[(size_t)v * 2 + 1];
        const float bd2 = knn_box_d2(q.x, q.y, q.z, lo, hi);
        if (__ballot(valid && bd2 < top.d[K - 1]) == 0) continue;
        if (v >= p2) {
            knn_scan_leaf<K>(pts, v - p2, q.x, q.y, q.z, self, top);
            ++nleaf;
            continue;
        }
        // children of v cover leaves [lo_leaf, lo_leaf + span); the half holding (or nearer in Morton order to) the
        // wave's own leaf is popped first.  The own leaf itself is never pushed.
        const int lvl = 31 - __builtin_clz(v);                       // depth of v
        const int span = p2 >> (lvl + 1);                            // leaves under each child
        const int mid = (v << (31 - __builtin_clz(p2) - lvl)) - p2 + span;
        const int cl = 2 * v, cr = 2 * v + 1;
        const int first = leaf < mid ? cl : cr, second = leaf < mid ? cr : cl;
        // at most one pending sibling per level plus the pair just pushed: <= levels + 1 < KNN_STACK entries.  Every
        // lane stores the same value, so each lane's later read follows its own store in program order.
        if (second != own) stack[sp++] = second;
        if (first != own) stack[sp++] = first;
    }

    if (visited && lane == 0) atomicAdd(visited, nleaf * KNN_LEAF * nvalid);
    if (!valid) return;
    const size_t row = (size_t)ids[self] * k;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        if (s >= K - k) {
            dist[row + s - (K - k)] = sqrtf(top.d[s]);
            idx[row + s - (K - k)] = top.j[s] >= 0 ? ids[top.j[s]] : -1;   // (-1 only for non-finite input)
        }
    }
}

template <int K>
void knn_query_launch(int n, int k, int leaves, int p2, const KnnLayout &L, float *dist, int32_t *idx,
                      int64_t *visited, hipStream_t s) {
    hipLaunchKernelGGL(knn_query<K>, dim3(sgn_cdiv(leaves, KNN_QUERY_WAVES)), dim3(64 * KNN_QUERY_WAVES), 0, s, n, k,
                       leaves, p2, L.pts, L.nodes, L.ids_out, dist, idx, (unsigned long long *)visited);
}

}  // namespace

SGN_EXPORT size_t sgn_knn_workspace_bytes(int n, int k) {
    (void)k;
    if (n <= 0 || n > KNN_MAX_N) return 0;
    return knn_layout(n, nullptr).total;
}

SGN_EXPORT int sgn_knn(int n, int k, const float *points, float *dist, int32_t *idx, int64_t *visited, void *ws,
                       size_t ws_bytes, sgn_stream_t stream) {
    SGN_ARG_CHECK(k >= 1 && k <= 16, -1);
    SGN_ARG_CHECK(n > k && n <= KNN_MAX_N, -2);
    SGN_ARG_CHECK(points && dist && idx && ws, -3);
    SGN_ARG_CHECK(ws_bytes >= sgn_knn_workspace_bytes(n, k), -4);
    hipStream_t s = (hipStream_t)stream;
    const KnnLayout L = knn_layout(n, ws);
    const int leaves = knn_leaves(n), p2 = knn_pow2(leaves);
    const int rc = knn_build_tree(n, points, L, nullptr, stream);
    if (rc != 0) return rc;
    switch (k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16) {
        case 1: knn_query_launch<1>(n, k, leaves, p2, L, dist, idx, visited, s); break;
        case 2: knn_query_launch<2>(n, k, leaves, p2, L, dist, idx, visited, s); break;
        case 4: knn_query_launch<4>(n, k, leaves, p2, L, dist, idx, visited, s); break;
        case 8: knn_query_launch<8>(n, k, leaves, p2, L, dist, idx, visited, s); break;
        default: knn_query_launch<16>(n, k, leaves, p2, L, dist, idx, visited, s); break;
    }
    SGN_LAUNCH_CHECK();
    return 0;
}
