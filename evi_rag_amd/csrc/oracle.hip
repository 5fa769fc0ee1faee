// Retriever-oracle answer hits over ranked triplet windows (src/models/reasoner_module.py:17-68).
//
//   k_oracle_hits   one workgroup per sample: the answer ids are sorted (bitonic) in LDS, or in a workspace region when
//                   they do not fit; every rank r < min(E, max_scan_k) looks its head and tail up by binary search and
//                   lowers first_rank[slot] of the answer it hits (atomicMin); then, per k, the distinct answers whose
//                   first rank is below k are counted.
//
// The reference walks the ranks one by one with a Python set of found answers and reads the state at each k.  "The
// answer's first rank is < k" is that state without the walk: duplicate answers share the slot of their first sorted
// occurrence, a head and a tail hitting one answer lower the same slot, and a k past the end of the list sees every
// rank scanned, which is the reference's "k beyond the list carries the last value".  Nothing depends on the order in
// which the ranks are visited.
//
// The data are a few hundred ids per sample: bound by latency (barriers of the sort, dependent LDS loads of the
// searches), not by bandwidth.
#include "common.hpp"

#include <limits.h>

namespace evi {
namespace {

constexpr int kOracleThreads = 256;
constexpr int kOracleWaves = kOracleThreads / 64;
constexpr int kSlotBytes = 8 + 4;                // sorted answer id + first rank
constexpr int kMaxLdsAnswers = 4096;             // 48 KiB: three workgroups of 256 threads per CU still fit
constexpr int64_t kMaxAnswersPerCall = 1ll << 30;

struct OracleArgs {
    const int64_t* edge_ptr;
    const int64_t* head;
    const int64_t* tail;
    const int64_t* answer_ptr;
    const int64_t* answers;
    int32_t* uniq;
    int32_t* found;
    int64_t* ws_keys;   // [2 * total_answers]: sample s owns [2 * answer_ptr[s], ...) when it does not fit in LDS
    int32_t* ws_first;  // [2 * total_answers]
    int nk;
    int max_scan_k;
    int lds_answers;
    int ks[EVI_ORACLE_MAX_KS];
};

__device__ __forceinline__ int next_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// Sum over the workgroup; every thread gets the total.  `red` holds one int per wave.
__device__ __forceinline__ int block_sum(int v, int* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < kOracleWaves; ++w) total += red[w];
    __syncthreads();
    return total;
}

// First index i in [0, n) with keys[i] >= x (n when none).
__device__ __forceinline__ int lower_bound(const int64_t* keys, int n, int64_t x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// One sample over `keys` / `first` (P slots each, LDS or its workspace region).  P, na and scan are uniform over the
// workgroup, so every barrier below is reached by all threads.
__device__ __forceinline__ void oracle_sample(const OracleArgs& a, int s, int64_t* keys, int32_t* first, int na, int P,
                                              int64_t a0, int64_t e0, int scan, int* red) {
    const int tid = threadIdx.x;
    for (int i = tid; i < P; i += kOracleThreads) {
        keys[i] = i < na ? a.answers[a0 + i] : INT64_MAX;  // padding sorts last; only [0, na) is read afterwards
        first[i] = INT_MAX;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += kOracleThreads) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const int64_t x = keys[i], y = keys[ixj];
                    if ((x > y) == ((i & k) == 0)) {
                        keys[i] = y;
                        keys[ixj] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    // ranks 0 .. scan-1: a hit lowers the first rank of the answer's first sorted occurrence
    for (int r = tid; r < scan; r += kOracleThreads) {
        const int64_t h = a.head[e0 + r];
        const int64_t t = a.tail[e0 + r];
        const int ph = lower_bound(keys, na, h);
        if (ph < na && keys[ph] == h) atomicMin(&first[ph], r);
        const int pt = lower_bound(keys, na, t);
        if (pt < na && keys[pt] == t) atomicMin(&first[pt], r);
    }
    __syncthreads();
    int u = 0;
    for (int i = tid; i < na; i += kOracleThreads) u += (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
    u = block_sum(u, red);
    if (tid == 0) a.uniq[s] = u;
    for (int q = 0; q < a.nk; ++q) {
        const int kk = a.ks[q];
        int c = 0;
        for (int i = tid; i < na; i += kOracleThreads) c += first[i] < kk ? 1 : 0;  // only first occurrences are ever set
        c = block_sum(c, red);
        if (tid == 0) a.found[(int64_t)s * a.nk + q] = c;
    }
}

__global__ __launch_bounds__(kOracleThreads) void k_oracle_hits(OracleArgs a) {
    extern __shared__ int64_t lds_keys[];
    __shared__ int red[kOracleWaves];
    const int s = blockIdx.x;
    const int64_t a0 = a.answer_ptr[s];
    const int na = (int)(a.answer_ptr[s + 1] - a0);
    const int64_t e0 = a.edge_ptr[s];
    const int64_t ne = a.edge_ptr[s + 1] - e0;
    const int scan = (int)(ne < (int64_t)a.max_scan_k ? ne : (int64_t)a.max_scan_k);
    const int P = na > 0 ? next_pow2(na) : 0;
    if (P <= a.lds_answers) {
        int32_t* lds_first = reinterpret_cast<int32_t*>(lds_keys + a.lds_answers);
        oracle_sample(a, s, lds_keys, lds_first, na, P, a0, e0, scan, red);
    } else {
        oracle_sample(a, s, a.ws_keys + 2 * a0, a.ws_first + 2 * a0, na, P, a0, e0, scan, red);
    }
}

}  // namespace
}  // namespace evi

using namespace evi;

namespace {
struct OracleLayout {
    size_t keys, first, total;
};

OracleLayout oracle_layout(int64_t total_answers) {
    // next_pow2(n) <= 2n, so a sample's region at 2 * answer_ptr[s] never reaches the next sample's
    Bump b;
    OracleLayout l;
    l.keys = b.take(sizeof(int64_t) * 2 * total_answers);
    l.first = b.take(sizeof(int32_t) * 2 * total_answers);
    l.total = b.total;
    return l;
}
}  // namespace

extern "C" {

size_t evi_oracle_answer_hits_workspace_bytes(int64_t total_answers) {
    if (total_answers <= 0 || total_answers >= kMaxAnswersPerCall) return 0;
    return oracle_layout(total_answers).total;
}

int evi_oracle_answer_hits(int num_samples, const int64_t* edge_ptr, const int64_t* head_ids, const int64_t* tail_ids,
                           const int64_t* answer_ptr, const int64_t* answer_ids, int64_t total_answers, const int64_t* ks_host,
                           int nk, int max_scan_k, int lds_answers, int32_t* uniq, int32_t* found, void* workspace,
                           size_t workspace_bytes, void* stream) {
    EVI_REQUIRE(num_samples >= 0, "evi_oracle_answer_hits: num_samples must be >= 0, got %d", num_samples);
    EVI_REQUIRE(ks_host, "evi_oracle_answer_hits: null ks_host");
    EVI_REQUIRE(nk >= 1 && nk <= EVI_ORACLE_MAX_KS, "evi_oracle_answer_hits: nk must be in [1, %d], got %d", EVI_ORACLE_MAX_KS,
                nk);
    for (int q = 0; q < nk; ++q) {
        EVI_REQUIRE(ks_host[q] >= 1, "evi_oracle_answer_hits: ks must be positive, ks[%d] = %lld", q, (long long)ks_host[q]);
        EVI_REQUIRE(q == 0 || ks_host[q] > ks_host[q - 1], "evi_oracle_answer_hits: ks must be strictly ascending, ks[%d] = %lld "
                    "after %lld", q, (long long)ks_host[q], (long long)ks_host[q - 1]);
    }
    EVI_REQUIRE(max_scan_k >= 0, "evi_oracle_answer_hits: max_scan_k must be >= 0, got %d", max_scan_k);
    EVI_REQUIRE(total_answers >= 0 && total_answers < kMaxAnswersPerCall,
                "evi_oracle_answer_hits: total_answers must be in [0, 2^30), got %lld", (long long)total_answers);
    EVI_REQUIRE(lds_answers >= 0 && lds_answers <= kMaxLdsAnswers, "evi_oracle_answer_hits: lds_answers must be in [0, %d], got %d",
                kMaxLdsAnswers, lds_answers);
    if (num_samples == 0) return EVI_OK;
    EVI_REQUIRE(edge_ptr && head_ids && tail_ids && answer_ptr && uniq && found,
                "evi_oracle_answer_hits: null offset, id or output pointer");
    EVI_REQUIRE(total_answers == 0 || answer_ids, "evi_oracle_answer_hits: null answer_ids");
    const OracleLayout l = oracle_layout(total_answers);
    EVI_REQUIRE(total_answers == 0 || (workspace && workspace_bytes >= l.total),
                "evi_oracle_answer_hits: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    OracleArgs a{};
    a.edge_ptr = edge_ptr;
    a.head = head_ids;
    a.tail = tail_ids;
    a.answer_ptr = answer_ptr;
    a.answers = answer_ids;
    a.uniq = uniq;
    a.found = found;
    char* ws = static_cast<char*>(workspace);
    a.ws_keys = total_answers ? reinterpret_cast<int64_t*>(ws + l.keys) : nullptr;
    a.ws_first = total_answers ? reinterpret_cast<int32_t*>(ws + l.first) : nullptr;
    a.nk = nk;
    a.max_scan_k = max_scan_k;
    a.lds_answers = lds_answers;
    for (int q = 0; q < nk; ++q) a.ks[q] = ks_host[q] > INT_MAX ? INT_MAX : (int)ks_host[q];  // first ranks are < INT_MAX
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    static bool attr_set = false;
    if (!attr_set) {
        EVI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_oracle_hits),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsAnswers * kSlotBytes));
        attr_set = true;
    }
    hipLaunchKernelGGL(k_oracle_hits, dim3(num_samples), dim3(kOracleThreads), (size_t)lds_answers * kSlotBytes, st, a);
    EVI_LAUNCH_CHECK();
    return EVI_OK;
}

}  // extern "C"
