// Canonical positive edges of a whole batch: among the parallel positive edges of one unordered node pair
// keep the edge whose relation is most cosine-similar to the graph's question, then re-filter the (seed, answer) pair lists.
//   evi_canonical_edges pass 0   _group_positive_edges_by_pair + _select_canonical_edge_indices + the counts of _filter_pair_edges
//   evi_canonical_edges pass 1   the ids of _filter_pair_edges
// reference: scripts/build_retrieval_pipeline.py:840-932.
//
// One workgroup per graph.  The positives are gathered into a small table (node pair, relation id, edge id), a permutation of the
// table is bitonic-sorted by (lo, hi, relation id, edge id), and a group is a run of equal (lo, hi) in that order: its first
// maximum is the reference's argmax over `sorted(members, key=(relation_id, idx))`.  Only members of runs of two or more are
// scored, one wave per member.  The table lives in LDS up to kCanonLdsCap positives and in the caller's workspace beyond.
#include "common.hpp"

namespace evi {

constexpr int kCanonThreads = 256;
constexpr int kCanonWaves = kCanonThreads / 64;
constexpr int kCanonLdsCap = 1024;        // positives of one graph that fit the LDS table (48 B each: 48 KiB, three graphs per CU)
constexpr size_t kCanonItemBytes = 48;    // lo, hi, rel, eid, best (8 B each) + perm, todo (4 B each)

// The table of one graph, structure of arrays over `cap` slots (cap a power of two >= the number of positives).
struct CanonTable {
    int64_t* lo;      // [cap] min(u, v) of the slot's edge
    int64_t* hi;      // [cap] max(u, v)
    int64_t* rel;     // [cap] relation id as given
    int64_t* eid;     // [cap] batch-global edge id
    uint64_t* best;   // [cap] per sorted position of a group's head: max over the members of (ordered score, ~sorted position)
    int32_t* perm;    // [cap] sorted position -> slot
    int32_t* todo;    // [cap] sorted positions that need a score
    __device__ CanonTable(void* base, int64_t cap) {
        lo = reinterpret_cast<int64_t*>(base);
        hi = lo + cap;
        rel = hi + cap;
        eid = rel + cap;
        best = reinterpret_cast<uint64_t*>(eid + cap);
        perm = reinterpret_cast<int32_t*>(best + cap);
        todo = perm + cap;
    }
};

// relation row . question row.  Element j belongs to lane (j / 4) % 64 and a lane adds its elements in ascending j with one
// fused multiply-add each; the 64 partial sums meet in a butterfly (every lane ends with the same bits).  The vector form
// (VEC, D % 4 == 0 and 16-byte aligned rows) and the scalar form issue the same operations on the same values, so a score is a
// function of the two rows' bytes alone.
template <bool VEC>
__device__ inline float canon_dot(const float* __restrict__ r, const float* __restrict__ q, int D, int lane) {
    float acc = 0.0f;
    for (int j0 = 4 * lane; j0 < D; j0 += 256) {
        if (VEC) {
            const float4 a = *reinterpret_cast<const float4*>(r + j0);
            const float4 b = *reinterpret_cast<const float4*>(q + j0);
            acc = fmaf(a.x, b.x, acc);
            acc = fmaf(a.y, b.y, acc);
            acc = fmaf(a.z, b.z, acc);
            acc = fmaf(a.w, b.w, acc);
        } else {
            const int end = j0 + 4 < D ? j0 + 4 : D;
            for (int j = j0; j < end; ++j) acc = fmaf(r[j], q[j], acc);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    return acc;
}

// Order of the sort: real slots by (lo, hi, rel, eid), padding slots (>= n) after every real one.
__device__ inline bool canon_less(const CanonTable& t, int a, int b, int n) {
    if (a >= n || b >= n) return a < b;
    const int64_t la = t.lo[a], lb = t.lo[b];
    if (la != lb) return la < lb;
    const int64_t ha = t.hi[a], hb = t.hi[b];
    if (ha != hb) return ha < hb;
    const int64_t ra = t.rel[a], rb = t.rel[b];
    if (ra != rb) return ra < rb;
    return t.eid[a] < t.eid[b];
}

__device__ inline bool canon_same_pair(const CanonTable& t, int sa, int sb) { return t.lo[sa] == t.lo[sb] && t.hi[sa] == t.hi[sb]; }

// Everything after the count of positives, on a table in LDS or in the workspace (the same code; instantiated once for each so
// that the LDS form compiles to LDS instructions).  n positives, cap = next power of two >= n, `counter` two LDS ints.
template <bool VEC>
__device__ inline void canon_graph(CanonTable t, int n, int cap, int* counter, int64_t e0, int64_t e1, int64_t E,
                                   const int64_t* __restrict__ edge_index, const int64_t* __restrict__ edge_rel,
                                   const uint8_t* __restrict__ mask, const float* __restrict__ qrow,
                                   const float* __restrict__ relation_norm, int64_t R, int D, uint8_t* __restrict__ keep,
                                   int32_t* __restrict__ status) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < cap; i += kCanonThreads) {
        t.perm[i] = i;
        t.best[i] = 0ull;
    }
    __syncthreads();
    // gather (slot order is arbitrary: the sort key is total, so the sorted order does not depend on it)
    for (int64_t e = e0 + tid; e < e1; e += kCanonThreads) {
        if (mask[e] == 0) continue;
        const int s = atomicAdd(&counter[0], 1);
        if (s >= n) continue;  // cannot happen: n is the count of the same bytes
        const int64_t u = edge_index[e], v = edge_index[E + e];
        t.lo[s] = u < v ? u : v;
        t.hi[s] = u < v ? v : u;
        t.rel[s] = edge_rel[e];
        t.eid[s] = e;
    }
    // bitonic sort of perm, ascending
    for (int size = 2; size <= cap; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int x = tid; x < (cap >> 1); x += kCanonThreads) {
                const int i = 2 * x - (x & (stride - 1));
                const int j = i + stride;
                const int a = t.perm[i], b = t.perm[j];
                const bool asc = (i & size) == 0;
                const bool swap = asc ? canon_less(t, b, a, n) : canon_less(t, a, b, n);
                if (swap) {
                    t.perm[i] = b;
                    t.perm[j] = a;
                }
            }
        }
    }
    __syncthreads();
    // classify: a singleton keeps its edge unscored; members of longer runs are queued for a score
    for (int i = tid; i < n; i += kCanonThreads) {
        const int s = t.perm[i];
        const bool head = i == 0 || !canon_same_pair(t, t.perm[i - 1], s);
        const bool tail = i == n - 1 || !canon_same_pair(t, t.perm[i + 1], s);
        if (head && tail)
            keep[t.eid[s]] = 1;
        else
            t.todo[atomicAdd(&counter[1], 1)] = i;
    }
    __syncthreads();
    const int m = counter[1];
    for (int k = wave; k < m; k += kCanonWaves) {
        const int i = t.todo[k];
        const int s = t.perm[i];
        int64_t r = t.rel[s];
        const bool bad = r < 0 || r >= R;
        if (bad) r = r < 0 ? 0 : R - 1;  // scored clamped (never a read outside the table), reported through status
        const float score = R > 0 ? canon_dot<VEC>(relation_norm + r * (int64_t)D, qrow, D, lane) : 0.0f;
        if (lane == 0) {
            int flags = bad ? 1 : 0;
            if (!(fabsf(score) <= 3.402823466e+38f)) flags |= 2;
            if (flags) atomicOr(status, flags);
            // head of the run: the first sorted position with this node pair
            int lo = 0, hi = i;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const int sm = t.perm[mid];
                const bool before = t.lo[sm] != t.lo[s] ? t.lo[sm] < t.lo[s] : t.hi[sm] < t.hi[s];
                if (before)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            atomicMax(reinterpret_cast<unsigned long long*>(&t.best[lo]), (unsigned long long)make_key(score, (uint32_t)i));
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += kCanonThreads) {
        const uint64_t b = t.best[i];
        if (b != 0ull) keep[t.eid[t.perm[key_index(b)]]] = 1;
    }
}

template <bool VEC>
__global__ __launch_bounds__(kCanonThreads) void k_canonical_keep(
    const int64_t* __restrict__ edge_index, int64_t E, const int64_t* __restrict__ edge_ptr,
    const int64_t* __restrict__ edge_rel, const uint8_t* __restrict__ mask, const float* __restrict__ question_norm,
    const float* __restrict__ relation_norm, int64_t R, int D, uint8_t* __restrict__ keep, int32_t* __restrict__ status,
    uint8_t* __restrict__ workspace) {
    __shared__ __attribute__((aligned(16))) uint8_t lds_table[kCanonLdsCap * kCanonItemBytes];
    __shared__ int counter[2];
    __shared__ int wave_count[kCanonWaves];
    const int g = blockIdx.x, tid = threadIdx.x;
    int64_t e0 = edge_ptr[g], e1 = edge_ptr[g + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > E) e1 = E;
    int local = 0;
    for (int64_t e = e0 + tid; e < e1; e += kCanonThreads) {
        keep[e] = 0;
        local += mask[e] != 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) local += __shfl_xor(local, off, 64);
    if ((tid & 63) == 0) wave_count[tid >> 6] = local;
    if (tid < 2) counter[tid] = 0;
    __syncthreads();  // also orders the zeroes of `keep` before the ones written below
    int n = 0;
#pragma unroll
    for (int w = 0; w < kCanonWaves; ++w) n += wave_count[w];
    if (n == 0) return;
    int cap = 1;
    while (cap < n) cap <<= 1;
    const float* qrow = question_norm + (int64_t)g * D;
    if (n <= kCanonLdsCap)
        canon_graph<VEC>(CanonTable(lds_table, cap), n, cap, counter, e0, e1, E, edge_index, edge_rel, mask, qrow, relation_norm, R,
                         D, keep, status);
    else  // cap < 2 n <= 2 E_g: the graph's slice of the workspace starts at item 2 e0
        canon_graph<VEC>(CanonTable(workspace + 2 * e0 * (int64_t)kCanonItemBytes, cap), n, cap, counter, e0, e1, E, edge_index,
                         edge_rel, mask, qrow, relation_norm, R, D, keep, status);
}

// One wave per pair slot.  PASS 0: new_count[p] = ids of the pair's span whose keep is 1.  PASS 1: those ids, in the span's
// order, at new_ids[new_off[p] ...].  An id outside [0, E) is dropped.
template <int PASS>
__global__ __launch_bounds__(kCanonThreads) void k_canonical_pairs(
    const int32_t* __restrict__ pair_count, const int64_t* __restrict__ pair_edge_off, const int64_t* __restrict__ pair_edge_ids,
    int num_pairs, int64_t E, const uint8_t* __restrict__ keep, int32_t* __restrict__ new_count,
    const int64_t* __restrict__ new_off, int64_t* __restrict__ new_ids) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * kCanonWaves + (threadIdx.x >> 6);
    if (p >= num_pairs) return;
    const int64_t b = pair_edge_off[p];
    const int c = pair_count[p];
    int64_t out = PASS == 1 ? new_off[p] : 0;
    int total = 0;
    for (int c0 = 0; c0 < c; c0 += 64) {
        const int x = c0 + lane;
        int64_t id = -1;
        if (x < c) id = pair_edge_ids[b + x];
        const bool kept = id >= 0 && id < E && keep[id] != 0;
        const unsigned long long ballot = __ballot(kept);
        if (PASS == 1 && kept) new_ids[out + total + __popcll(ballot & ((1ull << lane) - 1ull))] = id;
        total += __popcll(ballot);
    }
    if (PASS == 0 && lane == 0) new_count[p] = total;
}

}  // namespace evi

using namespace evi;

extern "C" int evi_canonical_edges_lds_capacity(void) { return kCanonLdsCap; }

extern "C" size_t evi_canonical_edges_workspace_bytes(int64_t E, int B, int D) {
    (void)B;
    (void)D;
    if (E < 0) E = 0;
    return align_up(2 * (size_t)E * kCanonItemBytes, 256) + 256;
}

extern "C" int evi_canonical_edges(int pass, const int64_t* edge_index, int64_t E, const int64_t* edge_ptr, int B,
                                   const int64_t* edge_relation_ids, const uint8_t* mask, const int32_t* pair_count,
                                   const int64_t* pair_edge_off, const int64_t* pair_edge_ids, int num_pairs,
                                   const float* question_norm, const float* relation_norm, int64_t R, int D, uint8_t* keep,
                                   int32_t* new_pair_count, const int64_t* new_pair_edge_off, int64_t* new_pair_edge_ids,
                                   int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    EVI_REQUIRE(pass == 0 || pass == 1, "evi_canonical_edges: pass must be 0 (keep + counts) or 1 (fill)");
    EVI_REQUIRE(E >= 0 && B >= 0 && num_pairs >= 0 && R >= 0 && D >= 1, "evi_canonical_edges: bad sizes");
    EVI_REQUIRE(E == 0 || keep, "evi_canonical_edges: null keep");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int pair_blocks = (num_pairs + kCanonWaves - 1) / kCanonWaves;
    if (pass == 0) {
        if (B > 0 && E > 0) {
            EVI_REQUIRE(edge_index && edge_ptr && edge_relation_ids && mask && question_norm && status && (R == 0 || relation_norm),
                        "evi_canonical_edges: null pointer");
            if (workspace_bytes < evi_canonical_edges_workspace_bytes(E, B, D) || !workspace)
                return fail(EVI_ERR_NOMEM, "evi_canonical_edges: workspace of %zu bytes, need %zu", workspace_bytes,
                            evi_canonical_edges_workspace_bytes(E, B, D));
            EVI_REQUIRE(((uintptr_t)workspace & 7) == 0, "evi_canonical_edges: workspace must be 8-byte aligned");
            const bool vec = D % 4 == 0 && ((uintptr_t)question_norm & 15) == 0 && ((uintptr_t)relation_norm & 15) == 0;
            if (vec)
                hipLaunchKernelGGL(k_canonical_keep<true>, dim3(B), dim3(kCanonThreads), 0, st, edge_index, E, edge_ptr,
                                   edge_relation_ids, mask, question_norm, relation_norm, R, D, keep, status,
                                   static_cast<uint8_t*>(workspace));
            else
                hipLaunchKernelGGL(k_canonical_keep<false>, dim3(B), dim3(kCanonThreads), 0, st, edge_index, E, edge_ptr,
                                   edge_relation_ids, mask, question_norm, relation_norm, R, D, keep, status,
                                   static_cast<uint8_t*>(workspace));
            EVI_LAUNCH_CHECK();
        }
        if (num_pairs > 0) {
            EVI_REQUIRE(pair_count && pair_edge_off && new_pair_count, "evi_canonical_edges: null pair arrays");
            hipLaunchKernelGGL(k_canonical_pairs<0>, dim3(pair_blocks), dim3(kCanonThreads), 0, st, pair_count, pair_edge_off,
                               pair_edge_ids, num_pairs, E, keep, new_pair_count, new_pair_edge_off, new_pair_edge_ids);
            EVI_LAUNCH_CHECK();
        }
    } else if (num_pairs > 0) {
        EVI_REQUIRE(pair_count && pair_edge_off && new_pair_edge_off && new_pair_edge_ids, "evi_canonical_edges: null pair arrays");
        hipLaunchKernelGGL(k_canonical_pairs<1>, dim3(pair_blocks), dim3(kCanonThreads), 0, st, pair_count, pair_edge_off,
                           pair_edge_ids, num_pairs, E, keep, new_pair_count, new_pair_edge_off, new_pair_edge_ids);
        EVI_LAUNCH_CHECK();
    }
    return EVI_OK;
}
