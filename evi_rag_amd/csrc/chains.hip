// BFS candidate chains over g_agent samples (src/data/components/bfs_chain_builder.py:49-311).
//
//   k_chain_adjacency  oriented adjacency per node: forward entries at the head, backward entries at the tail,
//                      ordered by (score desc, edge id asc, direction asc), truncated to max_branch_per_node
//   k_chain_expand     level-synchronous expansion from the seeds into (parent, adjacency entry, f64 score) records
//   k_chain_rank       signature de-duplication (64-bit hash, confirmed by full signature comparison), frequency,
//                      best chain per signature, and the (-freq, -length, -score, first occurrence) order; top M out
//
// One workgroup per sample in every kernel.  The data are a few thousand integers per sample that live in LDS or L2:
// bound by latency (barriers between levels, ancestor walks, sort stages) and LDS capacity, not by HBM bandwidth.
//
// An adjacency entry is packed as (sample-local edge id << 1) | direction; direction 1 walks the edge tail -> head.
// A chain record is (parent record or -1, adjacency entry, score): its steps are recovered by walking the parents.
#include "common.hpp"

#include <limits.h>

namespace evi {
namespace {

constexpr int kChainThreads = 256;
constexpr int kChainWaves = kChainThreads / 64;
constexpr int kRecordLdsBytes = 4 + 4 + 8 + 4;  // parent, entry, score, child count
constexpr int kMaxDynamicLds = 160 * 1024 - 1024;  // the rest of the 160 KiB: the kernels' static scan scratch
constexpr int kMaxLdsRecords = kMaxDynamicLds / kRecordLdsBytes;
constexpr int kMaxLdsSortSlots = 32768;  // u32 each: 128 KiB
constexpr uint32_t kSentinel = 0xFFFFFFFFu;

struct ChainArgs {
    const int64_t* node_ptr;
    const int64_t* edge_ptr;
    const int64_t* seed_ptr;
    const int64_t* rec_ptr;
    const int64_t* sort_ptr;
    const int32_t* head;
    const int32_t* tail;
    const float* score;
    const int64_t* relation;
    const int64_t* entity;
    const int32_t* seeds;
    int max_len, min_len, max_total, allow_backward, max_branch, forbid_edge, forbid_node;
    int max_out, lds_records, lds_sort_slots;
    uint64_t hash_mask;
    // workspace
    int32_t* adj_cnt;
    int32_t* adj_start;
    int32_t* adj_len;
    int32_t* adj_raw;
    int32_t* adj_sorted;
    int32_t* rec_par;
    int32_t* rec_ent;
    double* rec_sc;
    int32_t* rec_cnt;
    uint64_t* dd_hash;
    int32_t* dd_len;
    int32_t* dd_rep;
    int32_t* dd_freq;
    int32_t* dd_best;
    int32_t* dd_gs;
    uint32_t* perm;
    // outputs
    int32_t* out_count;
    int32_t* out_len;
    int32_t* out_freq;
    double* out_score;
    int32_t* out_steps;
    int64_t* out_stats;  // [S][4]: records needed past the capacity (0: fitted), levels, raw chains, candidates
};

__device__ inline uint64_t chain_mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

__device__ inline int64_t wave_incl_sum(int64_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

__device__ inline int32_t wave_incl_max(int32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v = max(v, t);
    }
    return v;
}

// In-place exclusive sum over a[0, n) (values >= 0); offsets past INT32_MAX are clamped (they only ever meet bounds far
// below).  Every thread of the workgroup calls it and gets the 64-bit total.
__device__ int64_t block_scan_excl(int32_t* a, int n, int64_t* wsum) {
    const int tid = threadIdx.x, wave = tid >> 6;
    int64_t carry = 0;
    for (int base = 0; base < n; base += kChainThreads) {
        const int i = base + tid;
        const int64_t v = i < n ? a[i] : 0;
        const int64_t inc = wave_incl_sum(v);
        if ((tid & 63) == 63) wsum[wave] = inc;
        __threadfence_block();
        __syncthreads();
        int64_t before = carry, tile = 0;
#pragma unroll
        for (int w = 0; w < kChainWaves; ++w) {
            if (w < wave) before += wsum[w];
            tile += wsum[w];
        }
        if (i < n) a[i] = (int32_t)min(before + inc - v, (int64_t)INT_MAX);
        carry += tile;
        __threadfence_block();
        __syncthreads();
    }
    return carry;
}

// In-place inclusive max over a[0, n).
__device__ void block_scan_max(int32_t* a, int n, int32_t* wmax) {
    const int tid = threadIdx.x, wave = tid >> 6;
    int32_t carry = INT_MIN;
    for (int base = 0; base < n; base += kChainThreads) {
        const int i = base + tid;
        const int32_t inc = wave_incl_max(i < n ? a[i] : INT_MIN);
        if ((tid & 63) == 63) wmax[wave] = inc;
        __threadfence_block();
        __syncthreads();
        int32_t before = carry, tile = carry;
#pragma unroll
        for (int w = 0; w < kChainWaves; ++w) {
            if (w < wave) before = max(before, wmax[w]);
            tile = max(tile, wmax[w]);
        }
        if (i < n) a[i] = max(before, inc);
        carry = tile;
        __threadfence_block();
        __syncthreads();
    }
}

// Bitonic sort of v[0, P) (P a power of two) under a strict total order `less`; kSentinel sorts last.
template <class Less>
__device__ void block_bitonic_sort(uint32_t* v, int P, Less less) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += kChainThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const uint32_t a = v[i], b = v[l];
                    const bool b_first = (b != kSentinel) && (a == kSentinel || less(b, a));
                    if (b_first == ((i & k) == 0)) {
                        v[i] = b;
                        v[l] = a;
                    }
                }
            }
            __threadfence_block();
            __syncthreads();
        }
    }
}

struct SampleView {
    int64_t n0, e0;
    const int32_t* head;
    const int32_t* tail;
    __device__ inline int edge(int32_t x) const { return x >> 1; }
    __device__ inline int dst(int32_t x) const { return (x & 1) ? head[x >> 1] : tail[x >> 1]; }
    __device__ inline int src(int32_t x) const { return (x & 1) ? tail[x >> 1] : head[x >> 1]; }
};

// ---- adjacency ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kChainThreads) void k_chain_adjacency(ChainArgs a) {
    __shared__ int64_t wsum[kChainWaves];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int64_t n0 = a.node_ptr[s], e0 = a.edge_ptr[s];
    const int N = (int)(a.node_ptr[s + 1] - n0), E = (int)(a.edge_ptr[s + 1] - e0);
    const int32_t* head = a.head + e0;
    const int32_t* tail = a.tail + e0;
    const float* score = a.score + e0;
    int32_t* cnt = a.adj_cnt + n0;
    int32_t* start = a.adj_start + n0;
    int32_t* raw = a.adj_raw + 2 * e0;
    int32_t* sorted = a.adj_sorted + 2 * e0;
    for (int v = tid; v < N; v += kChainThreads) cnt[v] = 0;
    __threadfence_block();
    __syncthreads();
    for (int e = tid; e < E; e += kChainThreads) {
        atomicAdd(&cnt[head[e]], 1);
        if (a.allow_backward) atomicAdd(&cnt[tail[e]], 1);
    }
    __threadfence_block();
    __syncthreads();
    for (int v = tid; v < N; v += kChainThreads) start[v] = __hip_atomic_load(&cnt[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __threadfence_block();
    __syncthreads();
    block_scan_excl(start, N, wsum);
    for (int v = tid; v < N; v += kChainThreads) {
        const int deg = __hip_atomic_load(&cnt[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        a.adj_len[n0 + v] = (a.max_branch >= 0 && a.max_branch < deg) ? a.max_branch : deg;
        cnt[v] = start[v];  // now the fill cursor
    }
    __threadfence_block();
    __syncthreads();
    // unordered fill; the order within a node is fixed below by ranking, so the atomics' interleaving does not matter
    for (int e = tid; e < E; e += kChainThreads) {
        raw[atomicAdd(&cnt[head[e]], 1)] = e << 1;
        if (a.allow_backward) raw[atomicAdd(&cnt[tail[e]], 1)] = (e << 1) | 1;
    }
    __threadfence_block();
    __syncthreads();
    const int entries = a.allow_backward ? 2 * E : E;
    const SampleView g{n0, e0, head, tail};
    for (int p = tid; p < entries; p += kChainThreads) {
        const int32_t x = raw[p];
        const int v = g.src(x);
        const int b = start[v];
        const int end = __hip_atomic_load(&cnt[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const float sx = score[x >> 1];
        int rank = 0;
        for (int q = b; q < end; ++q) {
            const int32_t y = raw[q];
            const float sy = score[y >> 1];
            rank += (sy > sx || (sy == sx && y < x)) ? 1 : 0;  // (-score, edge id, direction); -0.0 == +0.0
        }
        sorted[b + rank] = x;
    }
}

// ---- expansion ------------------------------------------------------------------------------------------------------
struct Records {
    int32_t* par;
    int32_t* ent;
    double* sc;
    int32_t* cnt;
};

// May entry y (from node `last`) extend chain c?  Walks the chain's records back to its seed.
__device__ inline bool may_extend(const ChainArgs& a, const SampleView& g, const Records& r, int c, int32_t y) {
    if (!a.forbid_edge && !a.forbid_node) return true;
    const int ey = y >> 1, dy = g.dst(y);
    for (int q = c; q >= 0; q = r.par[q]) {
        const int32_t x = r.ent[q];
        if (a.forbid_edge && (x >> 1) == ey) return false;
        if (a.forbid_node && (g.dst(x) == dy || (r.par[q] < 0 && g.src(x) == dy))) return false;
    }
    return true;
}

__global__ __launch_bounds__(kChainThreads) void k_chain_expand(ChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ int64_t wsum[kChainWaves];
    __shared__ int overflow_flag;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int64_t n0 = a.node_ptr[s], e0 = a.edge_ptr[s], q0 = a.seed_ptr[s], r0 = a.rec_ptr[s];
    const int N = (int)(a.node_ptr[s + 1] - n0);
    const int Q = (int)(a.seed_ptr[s + 1] - q0);
    const int C = (int)(a.rec_ptr[s + 1] - r0);
    const SampleView g{n0, e0, a.head + e0, a.tail + e0};
    const float* score = a.score + e0;
    const int32_t* adj_start = a.adj_start + n0;
    const int32_t* adj_len = a.adj_len + n0;
    const int32_t* adj = a.adj_sorted + 2 * e0;
    const int32_t* seeds = a.seeds + q0;

    const bool in_lds = C <= a.lds_records;
    Records r;
    if (in_lds) {
        r.sc = reinterpret_cast<double*>(lds_raw);
        r.par = reinterpret_cast<int32_t*>(r.sc + C);
        r.ent = r.par + C;
        r.cnt = r.ent + C;
    } else {
        r.sc = a.rec_sc + r0;
        r.par = a.rec_par + r0;
        r.ent = a.rec_ent + r0;
        r.cnt = a.rec_cnt + r0;
    }
    const int64_t kNoLimit = INT64_MAX;
    const int first_out_level = a.min_len > 1 ? a.min_len : 1;

    // level 1: every adjacency entry of every in-range seed, seeds in file order (duplicates kept)
    int64_t overflow = 0;
    int hi = 0, out_first = 0, levels = 0;
    {
        // child counts of the seeds go to cnt[0, Q) -- C >= Q is guaranteed by the host, or the counts go to rec_cnt
        int32_t* sc_cnt = (Q <= C) ? r.cnt : nullptr;
        if (sc_cnt == nullptr) {
            if (tid == 0) overflow_flag = 1;
        } else {
            if (tid == 0) overflow_flag = 0;
            for (int i = tid; i < Q; i += kChainThreads) {
                const int v = seeds[i];
                sc_cnt[i] = (v >= 0 && v < N) ? adj_len[v] : 0;
            }
        }
        __threadfence_block();
        __syncthreads();
        if (overflow_flag) {
            overflow = (int64_t)Q;
        } else {
            const int64_t total = block_scan_excl(sc_cnt, Q, wsum);
            const int64_t limit = (a.max_total > 0 && 1 >= a.min_len) ? (int64_t)a.max_total : kNoLimit;
            const int64_t need = min(total, limit);
            if (need > C) {
                overflow = need;
            } else {
                const int n = (int)need;
                // each seed's entries go to [off, off + deg); the counts live in r.cnt, apart from the records
                for (int i = tid; i < Q; i += kChainThreads) {
                    const int v = seeds[i];
                    if (v < 0 || v >= N) continue;
                    const int off = sc_cnt[i];
                    const int deg = adj_len[v];
                    const int b = adj_start[v];
                    for (int j = 0; j < deg && off + j < n; ++j) {
                        const int32_t x = adj[b + j];
                        r.par[off + j] = -1;
                        r.ent[off + j] = x;
                        r.sc[off + j] = (double)score[x >> 1];
                    }
                }
                __threadfence_block();
                __syncthreads();
                hi = n;
                levels = n > 0 ? 1 : 0;
            }
        }
    }
    int lo = 0, level = 1;
    int64_t out_count = (first_out_level <= 1) ? hi : 0;
    if (first_out_level > 1) out_first = hi;
    while (overflow == 0 && level < a.max_len && hi > lo && !(a.max_total > 0 && out_count >= a.max_total)) {
        const int width = hi - lo;
        for (int i = tid; i < width; i += kChainThreads) {
            const int c = lo + i;
            const int v = g.dst(r.ent[c]);
            const int b = adj_start[v], deg = adj_len[v];
            int k = 0;
            for (int j = 0; j < deg; ++j) k += may_extend(a, g, r, c, adj[b + j]) ? 1 : 0;
            r.cnt[c] = k;
        }
        __threadfence_block();
        __syncthreads();
        const int64_t total = block_scan_excl(r.cnt + lo, width, wsum);
        const bool output_level = level + 1 >= first_out_level;
        const int64_t limit = (a.max_total > 0 && output_level) ? (int64_t)a.max_total - out_count : kNoLimit;
        const int64_t need = min(total, limit);
        if ((int64_t)hi + need > C) {
            overflow = (int64_t)hi + need;
            break;
        }
        const int n = (int)need;
        for (int i = tid; i < width; i += kChainThreads) {
            const int c = lo + i;
            int off = r.cnt[c];
            if (off >= n) continue;
            const int32_t xc = r.ent[c];
            const int v = g.dst(xc);
            const int b = adj_start[v], deg = adj_len[v];
            const double base = r.sc[c];
            for (int j = 0; j < deg && off < n; ++j) {
                const int32_t y = adj[b + j];
                if (!may_extend(a, g, r, c, y)) continue;
                r.par[hi + off] = c;
                r.ent[hi + off] = y;
                r.sc[hi + off] = base + (double)score[y >> 1];  // parent + edge, in path order, as the reference adds
                ++off;
            }
        }
        __threadfence_block();
        __syncthreads();
        lo = hi;
        hi += n;
        ++level;
        if (n > 0) levels = level;
        if (level == first_out_level) out_first = lo;
        if (output_level) out_count += n;
    }
    if (overflow == 0 && level < first_out_level) out_first = hi;  // never reached an output level
    if (overflow == 0 && in_lds) {
        for (int i = tid; i < hi; i += kChainThreads) {
            a.rec_par[r0 + i] = r.par[i];
            a.rec_ent[r0 + i] = r.ent[i];
            a.rec_sc[r0 + i] = r.sc[i];
        }
    }
    if (tid == 0) {
        int64_t* st = a.out_stats + 4 * (int64_t)s;
        st[0] = overflow;
        st[1] = overflow ? 0 : levels;
        st[2] = overflow ? 0 : (int64_t)(hi - out_first);
        st[3] = (int64_t)out_first;  // consumed by k_chain_rank, replaced there by the candidate count
    }
}

// ---- de-duplication and ranking -------------------------------------------------------------------------------------
struct RankView {
    SampleView g;
    const int64_t* rel;  // sample's relations
    const int64_t* ent;  // sample's node entity ids
    const int32_t* par;  // records, sample base
    const int32_t* rec;
    int first;  // first output record
};

// Step triple of record q: (entity[src], relation, entity[dst]).
__device__ inline void step_of(const RankView& v, int q, int64_t& a, int64_t& b, int64_t& c) {
    const int32_t x = v.rec[q];
    a = v.ent[v.g.src(x)];
    b = v.rel[x >> 1];
    c = v.ent[v.g.dst(x)];
}

__device__ inline bool same_signature(const RankView& v, int ci, int cj, int len) {
    int p = v.first + ci, q = v.first + cj;
    for (int k = 0; k < len; ++k) {
        int64_t a0, b0, c0, a1, b1, c1;
        step_of(v, p, a0, b0, c0);
        step_of(v, q, a1, b1, c1);
        if (a0 != a1 || b0 != b1 || c0 != c1) return false;
        p = v.par[p];
        q = v.par[q];
    }
    return true;
}

__global__ __launch_bounds__(kChainThreads) void k_chain_rank(ChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_perm[];
    __shared__ int32_t wmax[kChainWaves];
    __shared__ int32_t cand_total;
    const int s = blockIdx.x, tid = threadIdx.x;
    int64_t* st = a.out_stats + 4 * (int64_t)s;
    const int64_t M = a.max_out;
    if (st[0] != 0) {  // the expansion did not fit: nothing to rank (the host sizes this sample again)
        if (tid == 0) {
            a.out_count[s] = 0;
            st[3] = 0;
        }
        return;
    }
    const int64_t n0 = a.node_ptr[s], e0 = a.edge_ptr[s], r0 = a.rec_ptr[s], p0 = a.sort_ptr[s];
    const int n = (int)st[2];
    const int first = (int)st[3];
    int P = 1;
    while (P < n) P <<= 1;
    const RankView v{SampleView{n0, e0, a.head + e0, a.tail + e0}, a.relation + e0, a.entity + n0, a.rec_par + r0,
                     a.rec_ent + r0, first};
    const double* sc = a.rec_sc + r0 + first;
    uint64_t* hsh = a.dd_hash + r0;
    int32_t* len = a.dd_len + r0;
    int32_t* rep = a.dd_rep + r0;
    int32_t* freq = a.dd_freq + r0;
    int32_t* best = a.dd_best + r0;
    int32_t* gs = a.dd_gs + r0;
    uint32_t* perm = (n > 0 && P <= a.lds_sort_slots) ? lds_perm : a.perm + p0;

    // signature hash: each step mixed with its position from the chain's end and the chain's length
    for (int i = tid; i < n; i += kChainThreads) {
        uint64_t h = 0;
        int L = 0;
        for (int q = first + i; q >= 0; q = v.par[q]) {
            int64_t x, y, z;
            step_of(v, q, x, y, z);
            uint64_t t = chain_mix64((uint64_t)x + 0x9e3779b97f4a7c15ull * (uint64_t)(L + 1));
            t = chain_mix64(t ^ (uint64_t)y);
            t = chain_mix64(t ^ (uint64_t)z);
            h += t;
            ++L;
        }
        hsh[i] = chain_mix64(h ^ (uint64_t)L) & a.hash_mask;
        len[i] = L;
    }
    for (int i = tid; i < P; i += kChainThreads) perm[i] = i < n ? (uint32_t)i : kSentinel;
    __threadfence_block();
    __syncthreads();
    block_bitonic_sort(perm, P, [&](uint32_t x, uint32_t y) { return hsh[x] < hsh[y] || (hsh[x] == hsh[y] && x < y); });

    // hash groups: start of each position's group
    for (int p = tid; p < n; p += kChainThreads) gs[p] = (p == 0 || hsh[perm[p]] != hsh[perm[p - 1]]) ? p : 0;
    __threadfence_block();
    __syncthreads();
    block_scan_max(gs, n, wmax);
    // representative: the first chain (in chain order) of the group with the same full signature
    for (int p = tid; p < n; p += kChainThreads) {
        const uint32_t c = perm[p];
        int r = (int)c;
        for (int q = gs[p]; q < p; ++q) {
            const uint32_t d = perm[q];
            if (len[d] == len[c] && same_signature(v, (int)d, (int)c, len[c])) {
                r = (int)d;
                break;
            }
        }
        rep[c] = r;
    }
    __threadfence_block();
    __syncthreads();
    // frequency and best chain (first with the strictly greatest score) of every representative
    for (int p = tid; p < n; p += kChainThreads) {
        const uint32_t c = perm[p];
        if (rep[c] != (int)c) continue;
        int f = 0, b = (int)c;
        double bs = sc[c];
        for (int q = p; q < n && hsh[perm[q]] == hsh[c]; ++q) {
            const uint32_t d = perm[q];
            if (rep[d] != (int)c) continue;
            ++f;
            if (sc[d] > bs) {
                bs = sc[d];
                b = (int)d;
            }
        }
        freq[c] = f;
        best[c] = b;
    }
    if (tid == 0) cand_total = 0;
    __threadfence_block();
    __syncthreads();
    int mine = 0;
    for (int p = tid; p < n; p += kChainThreads) {
        const uint32_t c = perm[p];
        const bool is_rep = rep[c] == (int)c;
        perm[p] = is_rep ? c : kSentinel;
        mine += is_rep ? 1 : 0;
    }
    atomicAdd(&cand_total, mine);
    __threadfence_block();
    __syncthreads();
    const int K = cand_total;
    block_bitonic_sort(perm, P, [&](uint32_t x, uint32_t y) {
        if (freq[x] != freq[y]) return freq[x] > freq[y];
        if (len[x] != len[y]) return len[x] > len[y];
        const double sx = sc[best[x]], sy = sc[best[y]];
        if (sx != sy) return sx > sy;  // -0.0 ties with +0.0
        return x < y;                   // first occurrence
    });
    const int out = (int)min((int64_t)K, M);
    const int maxL = a.max_len;
    for (int i = tid; i < out; i += kChainThreads) {
        const uint32_t c = perm[i];
        const int b = best[c];
        const int L = len[c];
        const int64_t o = (int64_t)s * M + i;
        a.out_len[o] = L;
        a.out_freq[o] = freq[c];
        a.out_score[o] = sc[b];
        int k = L - 1;
        for (int q = first + b; q >= 0; q = v.par[q]) a.out_steps[o * maxL + (k--)] = v.rec[q];
    }
    if (tid == 0) {
        a.out_count[s] = out;
        st[3] = K;
    }
}

}  // namespace
}  // namespace evi

using namespace evi;

namespace {
struct ChainLayout {
    size_t adj_cnt, adj_start, adj_len, adj_raw, adj_sorted, rec_par, rec_ent, rec_sc, rec_cnt, dd_hash, dd_len, dd_rep, dd_freq,
        dd_best, dd_gs, perm, total;
};

ChainLayout chain_layout(int64_t TN, int64_t TE, int64_t R, int64_t P) {
    Bump b;
    ChainLayout l;
    l.adj_cnt = b.take(sizeof(int32_t) * TN);
    l.adj_start = b.take(sizeof(int32_t) * TN);
    l.adj_len = b.take(sizeof(int32_t) * TN);
    l.adj_raw = b.take(sizeof(int32_t) * 2 * TE);
    l.adj_sorted = b.take(sizeof(int32_t) * 2 * TE);
    l.rec_par = b.take(sizeof(int32_t) * R);
    l.rec_ent = b.take(sizeof(int32_t) * R);
    l.rec_sc = b.take(sizeof(double) * R);
    l.rec_cnt = b.take(sizeof(int32_t) * R);
    l.dd_hash = b.take(sizeof(uint64_t) * R);
    l.dd_len = b.take(sizeof(int32_t) * R);
    l.dd_rep = b.take(sizeof(int32_t) * R);
    l.dd_freq = b.take(sizeof(int32_t) * R);
    l.dd_best = b.take(sizeof(int32_t) * R);
    l.dd_gs = b.take(sizeof(int32_t) * R);
    l.perm = b.take(sizeof(uint32_t) * P);
    l.total = b.total;
    return l;
}
}  // namespace

extern "C" {

size_t evi_bfs_chains_workspace_bytes(int64_t total_nodes, int64_t total_edges, int64_t total_records, int64_t total_sort_slots) {
    if (total_nodes < 0 || total_edges < 0 || total_records < 0 || total_sort_slots < 0) return 0;
    return chain_layout(total_nodes, total_edges, total_records, total_sort_slots).total;
}

int evi_bfs_chains(int num_samples, const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* seed_ptr,
                   const int64_t* rec_ptr, const int64_t* sort_ptr, int64_t total_nodes, int64_t total_edges,
                   int64_t total_records, int64_t total_sort_slots, const int32_t* edge_head, const int32_t* edge_tail,
                   const float* edge_score, const int64_t* edge_relation, const int64_t* node_entity, const int32_t* seeds,
                   int max_chain_length, int min_chain_length, int max_total_chains, int allow_backward,
                   int max_branch_per_node, int forbid_edge_revisit, int forbid_node_revisit, int max_out, int lds_records,
                   int lds_sort_slots, int hash_bits, int32_t* out_count, int32_t* out_len, int32_t* out_freq,
                   double* out_score, int32_t* out_steps, int64_t* out_stats, void* workspace, size_t workspace_bytes,
                   void* stream) {
    EVI_REQUIRE(num_samples >= 0, "evi_bfs_chains: num_samples must be >= 0, got %d", num_samples);
    EVI_REQUIRE(total_nodes >= 0 && total_edges >= 0 && total_records >= 0 && total_sort_slots >= 0,
                "evi_bfs_chains: totals must be >= 0");
    EVI_REQUIRE(total_edges < (1ll << 30), "evi_bfs_chains: %lld edges in one call exceed 2^30", (long long)total_edges);
    EVI_REQUIRE(max_chain_length >= 1 && max_chain_length <= EVI_BFS_CHAIN_MAX_LENGTH,
                "evi_bfs_chains: max_chain_length must be in [1, %d], got %d", EVI_BFS_CHAIN_MAX_LENGTH, max_chain_length);
    EVI_REQUIRE(max_out >= 0, "evi_bfs_chains: max_out must be >= 0, got %d", max_out);
    EVI_REQUIRE(lds_records >= 0 && lds_records <= kMaxLdsRecords,
                "evi_bfs_chains: lds_records must be in [0, %d], got %d", kMaxLdsRecords, lds_records);
    EVI_REQUIRE(lds_sort_slots >= 0 && lds_sort_slots <= kMaxLdsSortSlots,
                "evi_bfs_chains: lds_sort_slots must be in [0, %d], got %d", kMaxLdsSortSlots, lds_sort_slots);
    EVI_REQUIRE(hash_bits >= 1 && hash_bits <= 64, "evi_bfs_chains: hash_bits must be in [1, 64], got %d", hash_bits);
    if (num_samples == 0) return EVI_OK;
    EVI_REQUIRE(node_ptr && edge_ptr && seed_ptr && rec_ptr && sort_ptr && out_count && out_stats,
                "evi_bfs_chains: null offset or output pointer");
    EVI_REQUIRE(total_edges == 0 || (edge_head && edge_tail && edge_score && edge_relation),
                "evi_bfs_chains: null edge array");
    EVI_REQUIRE(total_nodes == 0 || node_entity, "evi_bfs_chains: null node_entity");
    EVI_REQUIRE(max_out == 0 || (out_len && out_freq && out_score && out_steps), "evi_bfs_chains: null output array");
    const ChainLayout l = chain_layout(total_nodes, total_edges, total_records, total_sort_slots);
    EVI_REQUIRE(workspace && workspace_bytes >= l.total, "evi_bfs_chains: workspace of %zu bytes, %zu needed", workspace_bytes,
                l.total);
    char* ws = static_cast<char*>(workspace);
    ChainArgs a{};
    a.node_ptr = node_ptr;
    a.edge_ptr = edge_ptr;
    a.seed_ptr = seed_ptr;
    a.rec_ptr = rec_ptr;
    a.sort_ptr = sort_ptr;
    a.head = edge_head;
    a.tail = edge_tail;
    a.score = edge_score;
    a.relation = edge_relation;
    a.entity = node_entity;
    a.seeds = seeds;
    a.max_len = max_chain_length;
    a.min_len = min_chain_length;
    a.max_total = max_total_chains;
    a.allow_backward = allow_backward ? 1 : 0;
    a.max_branch = max_branch_per_node;
    a.forbid_edge = forbid_edge_revisit ? 1 : 0;
    a.forbid_node = forbid_node_revisit ? 1 : 0;
    a.max_out = max_out;
    a.lds_records = lds_records;
    a.lds_sort_slots = lds_sort_slots;
    a.hash_mask = hash_bits == 64 ? ~0ull : ((1ull << hash_bits) - 1ull);
    a.adj_cnt = reinterpret_cast<int32_t*>(ws + l.adj_cnt);
    a.adj_start = reinterpret_cast<int32_t*>(ws + l.adj_start);
    a.adj_len = reinterpret_cast<int32_t*>(ws + l.adj_len);
    a.adj_raw = reinterpret_cast<int32_t*>(ws + l.adj_raw);
    a.adj_sorted = reinterpret_cast<int32_t*>(ws + l.adj_sorted);
    a.rec_par = reinterpret_cast<int32_t*>(ws + l.rec_par);
    a.rec_ent = reinterpret_cast<int32_t*>(ws + l.rec_ent);
    a.rec_sc = reinterpret_cast<double*>(ws + l.rec_sc);
    a.rec_cnt = reinterpret_cast<int32_t*>(ws + l.rec_cnt);
    a.dd_hash = reinterpret_cast<uint64_t*>(ws + l.dd_hash);
    a.dd_len = reinterpret_cast<int32_t*>(ws + l.dd_len);
    a.dd_rep = reinterpret_cast<int32_t*>(ws + l.dd_rep);
    a.dd_freq = reinterpret_cast<int32_t*>(ws + l.dd_freq);
    a.dd_best = reinterpret_cast<int32_t*>(ws + l.dd_best);
    a.dd_gs = reinterpret_cast<int32_t*>(ws + l.dd_gs);
    a.perm = reinterpret_cast<uint32_t*>(ws + l.perm);
    a.out_count = out_count;
    a.out_len = out_len;
    a.out_freq = out_freq;
    a.out_score = out_score;
    a.out_steps = out_steps;
    a.out_stats = out_stats;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    static bool attr_set = false;
    if (!attr_set) {
        EVI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_chain_expand),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds));
        EVI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_chain_rank),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds));
        attr_set = true;
    }
    hipLaunchKernelGGL(k_chain_adjacency, dim3(num_samples), dim3(kChainThreads), 0, st, a);
    EVI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_chain_expand, dim3(num_samples), dim3(kChainThreads), (size_t)lds_records * kRecordLdsBytes, st, a);
    EVI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_chain_rank, dim3(num_samples), dim3(kChainThreads), (size_t)lds_sort_slots * sizeof(uint32_t), st, a);
    EVI_LAUNCH_CHECK();
    return EVI_OK;
}

}  // extern "C"
