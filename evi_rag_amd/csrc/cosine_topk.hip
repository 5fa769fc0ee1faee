// Dense query x index cosine top-k for gfx950 (MI355X).
//
// Replaces (generalised from per-group arg-max to a global top-k) the arithmetic of
//   _normalize_embeddings + index_select + torch.mv + argmax
//   reference: scripts/build_retrieval_pipeline.py:833-837, 856-874.
//
// Data path
//   The index [N, D] f32 lives in HBM and is streamed exactly once per batch of <= 32 queries.
//   Each wave owns 16 index rows at a time and loads them straight into MFMA B-fragments
//   (lane (n = l&15, g = l>>4) reads 16 B of row n at column 16 j + 4 g): no LDS round trip for
//   the stream, which no other wave reuses.  The loads run one group ahead of the MFMAs, across
//   tile boundaries, and nothing on the common path waits for more than the group it multiplies.
//   The <= 32 queries are pre-fragmented once into the A-operand order and parked in LDS for the
//   whole launch (D * 128 B: 96 KiB at D = 768).
//   v_mfma_f32_16x16x4_f32 computes the [32 queries x 16 rows] block as an exact f32 FMA chain
//   in a fixed order of d, so a row's score never depends on where the row sits.
//
// Selection (exact)
//   Rows are scanned in segments of geometrically growing length.  The first segment writes its
//   scores densely; every later segment appends only rows whose score reaches the query's current
//   k-th best (tau), through a per-query atomic cursor.  After each segment one workgroup per
//   query selects the exact top-k of its candidate list (LDS bitonic sort, with an 8-bit radix
//   select in front when the list exceeds 8192 keys) and raises tau.  The candidate buffer holds
//   k + segment_rows entries, so it cannot overflow for any data (e.g. an index sorted by score).
//
// Bound: HBM.  Algorithmic bytes per batch = N*D*4 + N*4 (row_scale, optional) + Q*D*4 + Q*k*12.
#include "common.hpp"

#include <hip/hip_fp8.h>

#include <stdlib.h>

namespace evi {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kQueryBlock = 32;               // queries per pass over the index
constexpr int64_t kFirstSegment = 65536;      // dense segment: every score is written, no filter yet
constexpr int kCntStride = 64;                // one append cursor per 256 B: no false sharing between queries
constexpr int64_t kSegmentGrowth = 16;
constexpr int64_t kMaxSegmentDefault = 1 << 24;  // recommended workspace: 8 B x 32 x (min(N, 2^24) + k)

// How the index is stored and multiplied; the values are k_cosine_score's third template argument.
enum IndexKind : int {
    kIdxF32 = 0,       // f32 rows, exact f32 MFMA chain
    kIdxF16 = 1,       // f16 rows, query split hi + lo in f16
    kIdxFp8Widen = 2,  // e4m3 rows + row_scale, bytes widened to f16 in registers
    kIdxFp8Mfma = 3,   // e4m3 rows + row_scale on the native fp8 MFMA, query as two e4m3 pieces
};
static int index_chunks(IndexKind kind, int D) {  // 64-byte pieces of a row
    return kind >= kIdxFp8Widen ? D / 64 : (kind == kIdxF16 ? D / 32 : D / 16);
}
// bytes of nq queries' fragments: two 1-byte pieces per element for the native fp8 MFMA, 4 bytes per element otherwise
static size_t query_frag_bytes(IndexKind kind, int D, int nq) {
    return kind == kIdxFp8Mfma ? (size_t)D * 2 * nq : (size_t)D * nq * sizeof(float);
}

// Device-side gate: a scan enqueued as the FALLBACK of a proof-carrying fast path (two-stage scan) takes a pointer to that
// path's per-call status word; while the word is 0 (proof held) every kernel of the fallback returns at once, so the
// fallback costs a few empty launches and no read-back, and a failed proof is repaired on the device before anyone can
// consume the unproven result.  gate == nullptr: an ordinary, unconditional scan.
__device__ inline bool gate_closed(const int32_t* gate) {
    return gate != nullptr && *gate == 0;  // written by an earlier kernel of the same stream
}

// every query-fragment kernel also resets the batch's selection state (thresholds and append cursors): one launch
// fewer per batch than a separate reset kernel
__device__ inline void reset_query_state(float* tau, int32_t* cnt) {
    if (blockIdx.x == 0 && threadIdx.x < kQueryBlock) {
        tau[threadIdx.x] = -INFINITY;
        cnt[threadIdx.x * kCntStride] = 0;
    }
}

// q [Q, D] -> qfrag[((j*4 + g) * (NQB*16) + i) * 4 + t] = q[i][16 j + 4 g + t], zero for i >= Q.
__global__ void k_query_fragments(const float* __restrict__ q, int Q, int D, int nq_pad,
                                  float* __restrict__ qfrag, float* __restrict__ tau,
                                  int32_t* __restrict__ cnt, const int32_t* __restrict__ gate) {
    if (gate_closed(gate)) return;
    reset_query_state(tau, cnt);
    const int total = (D / 16) * 4 * nq_pad;  // float4 slots
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < total; s += gridDim.x * blockDim.x) {
        const int i = s % nq_pad;
        const int jg = s / nq_pad;  // j*4 + g
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < Q) v = *reinterpret_cast<const float4*>(q + (int64_t)i * D + jg * 4);
        reinterpret_cast<float4*>(qfrag)[s] = v;
    }
}

// f16-index variant: per K-step J of 32 and lane group g, the A fragment of query i is 8 halves
// q[i][32 J + 8 g .. + 7], stored twice: hi = f16(q) and lo = f16((q - hi) * 2048) (the scale keeps lo
// out of the f16 subnormal range; the lo accumulator is rescaled by 2^-11 at the end).
//   qfrag16[((J*4 + g)*2 + part) * nq_pad + i]  (16 bytes each), zero for i >= Q.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr float kLoScale = 2048.0f;
__global__ void k_query_fragments_f16(const float* __restrict__ q, int Q, int D, int nq_pad,
                                      f16x8* __restrict__ qfrag, float* __restrict__ tau,
                                      int32_t* __restrict__ cnt, const int32_t* __restrict__ gate) {
    if (gate_closed(gate)) return;
    reset_query_state(tau, cnt);
    const int total = (D / 32) * 4 * nq_pad;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < total; s += gridDim.x * blockDim.x) {
        const int i = s % nq_pad;
        const int jg = s / nq_pad;  // J*4 + g
        f16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = i < Q ? q[(int64_t)i * D + jg * 8 + e] : 0.f;
            const _Float16 h = (_Float16)v;
            hi[e] = h;
            lo[e] = (_Float16)((v - (float)h) * kLoScale);
        }
        qfrag[(jg * 2 + 0) * nq_pad + i] = hi;
        qfrag[(jg * 2 + 1) * nq_pad + i] = lo;
    }
}

// fp8-index variant: a 64-byte piece J of a row holds 64 e4m3 values; lane group g owns bytes
// 16 g .. 16 g + 15 and feeds them to two f16 MFMA K-steps (m = 0: bytes 0-7, m = 1: bytes 8-15).
//   qfrag8[(((J*2 + m)*4 + g)*2 + part) * nq_pad + i] = 8 halves of q[i][64 J + 16 g + 8 m .. + 7]
__global__ void k_query_fragments_fp8(const float* __restrict__ q, int Q, int D, int nq_pad,
                                      f16x8* __restrict__ qfrag, float* __restrict__ tau,
                                      int32_t* __restrict__ cnt, const int32_t* __restrict__ gate) {
    if (gate_closed(gate)) return;
    reset_query_state(tau, cnt);
    const int total = (D / 64) * 8 * nq_pad;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < total; s += gridDim.x * blockDim.x) {
        const int i = s % nq_pad;
        const int jmg = s / nq_pad;            // (J*2 + m)*4 + g
        const int g = jmg & 3, m = (jmg >> 2) & 1, J = jmg >> 3;
        f16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = i < Q ? q[(int64_t)i * D + 64 * J + 16 * g + 8 * m + e] : 0.f;
            const _Float16 h = (_Float16)v;
            hi[e] = h;
            lo[e] = (_Float16)((v - (float)h) * kLoScale);
        }
        qfrag[(jmg * 2 + 0) * nq_pad + i] = hi;
        qfrag[(jmg * 2 + 1) * nq_pad + i] = lo;
    }
}

// NATIVE fp8 MFMA variant (kIdxFp8Mfma): the e4m3 index bytes feed v_mfma_f32_16x16x32_fp8_fp8 as they are, so the query
// has to be fp8 too.  It is written as TWO e4m3 pieces with a power-of-two scale each,
//     q ~ s1 * p1 + s2 * p2,   p1 = e4m3(q / s1),  p2 = e4m3((q - s1 p1) / s2),
// (8 significant bits: |q - s1 p1 - s2 p2| <= 2^-8 |q|_inf per element, ~20x below the index's own e4m3 rounding), one
// accumulator per piece, recombined in the epilogue.  Same MFMA count as the widening variant (2 per k-step and query
// block) and no conversion work on the stream.  One workgroup per query (max |q| needs the whole row).
//   qfrag8n[((((J*2 + m)*4 + g)*2 + piece) * nq_pad + i] = 8 e4m3 bytes of piece(q[i])[64 J + 16 g + 8 m .. + 7]
//   qscale [piece][32] f32 behind the fragments (byte offset D * 2 * nq_pad)
__device__ inline float e4m3_to_float(uint32_t b) {
    const uint32_t e = (b >> 3) & 0xF, m = b & 7;
    const float mag = e == 0 ? (float)m * 0.001953125f /* 2^-9 */ : __uint_as_float(((e + 120u) << 23) | (m << 20));
    return (b & 0x80) ? -mag : mag;
}
__device__ inline float pow2_scale_for(float amax) {  // smallest power of two s with amax / s <= 448 (1 for amax == 0)
    if (!(amax > 0.f)) return 1.0f;
    int e;
    frexpf(amax / 448.0f, &e);  // amax / 448 = f * 2^e, f in [0.5, 1)
    return ldexpf(1.0f, e);
}
// THE two-piece form of a query, in one place: the fragment kernel of the native scan, the query planes of the many-query
// selection and the re-scoring chain all take a query's pieces and scales from these three functions, so they agree bit
// for bit.  A maximum does not depend on the order it is taken in, so `reduce_max` may be a workgroup's or a wave's.
__device__ inline uint32_t fp8n_piece1(float v, float s1) {
    return (uint32_t)__hip_cvt_float_to_fp8(v / s1, __HIP_SATFINITE, __HIP_E4M3) & 0xFF;
}
__device__ inline float fp8n_residual(float v, float s1, uint32_t b1) { return v - s1 * e4m3_to_float(b1); }
__device__ inline uint32_t fp8n_piece2(float v, float s1, uint32_t b1, float s2) {
    return (uint32_t)__hip_cvt_float_to_fp8(fp8n_residual(v, s1, b1) / s2, __HIP_SATFINITE, __HIP_E4M3) & 0xFF;
}
// s1, s2 of the query row q[0 .. D) (all zeros when !live), elements first, first + step, ... per caller thread
template <class ReduceMax>
__device__ inline void fp8n_query_scales(const float* __restrict__ q, int D, bool live, int first, int step,
                                         ReduceMax reduce_max, float& s1, float& s2) {
    float a1 = 0.f;
    for (int d = first; d < D; d += step) a1 = fmaxf(a1, live ? fabsf(q[d]) : 0.f);
    s1 = pow2_scale_for(reduce_max(a1));
    float a2 = 0.f;
    for (int d = first; d < D; d += step) {
        const float v = live ? q[d] : 0.f;
        a2 = fmaxf(a2, fabsf(fp8n_residual(v, s1, fp8n_piece1(v, s1))));
    }
    s2 = pow2_scale_for(reduce_max(a2));
}
// maximum over a 256-thread workgroup through red[256]
__device__ inline float block256_max(float* red, int tid, float v) {
    red[tid] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) red[tid] = fmaxf(red[tid], red[tid + off]);
        __syncthreads();
    }
    const float m = red[0];
    __syncthreads();
    return m;
}

__global__ __launch_bounds__(256) void k_query_fragments_fp8n(const float* __restrict__ q, int Q, int D, int nq_pad,
                                                              uint64_t* __restrict__ qfrag, float* __restrict__ tau,
                                                              int32_t* __restrict__ cnt, const int32_t* __restrict__ gate) {
    if (gate_closed(gate)) return;
    reset_query_state(tau, cnt);
    __shared__ float red[256];
    const int i = blockIdx.x, tid = threadIdx.x;  // one workgroup per query slot (grid = nq_pad)
    float* qscale = reinterpret_cast<float*>(reinterpret_cast<char*>(qfrag) + (size_t)D * 2 * nq_pad);
    const bool live = i < Q;
    float s1, s2;
    fp8n_query_scales(q + (int64_t)i * D, D, live, tid, 256, [&](float v) { return block256_max(red, tid, v); }, s1, s2);
    if (tid == 0) {
        qscale[i] = s1;
        qscale[kQueryBlock + i] = s2;
    }
    // 8 bytes per (J, m, g): thread -> one such group per trip
    const int groups = (D / 64) * 8;
    for (int jmg = tid; jmg < groups; jmg += 256) {
        const int g = jmg & 3, m = (jmg >> 2) & 1, J = jmg >> 3;
        uint64_t w1 = 0, w2 = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = live ? q[(int64_t)i * D + 64 * J + 16 * g + 8 * m + e] : 0.f;
            const uint32_t b1 = fp8n_piece1(v, s1);
            const uint32_t b2 = fp8n_piece2(v, s1, b1, s2);
            w1 |= (uint64_t)b1 << (8 * e);
            w2 |= (uint64_t)b2 << (8 * e);
        }
        qfrag[((int64_t)jmg * 2 + 0) * nq_pad + i] = w1;
        qfrag[((int64_t)jmg * 2 + 1) * nq_pad + i] = w2;
    }
}

// two e4m3 bytes of w (selected by `sel`) -> two f16 whose value is the fp8 value / 256:
// f16 bits = sign << 15 | (low 7 bits) << 7 (exact for every finite e4m3 code, subnormals included)
__device__ inline uint32_t fp8x2_to_f16x2_scaled(uint32_t w, uint32_t sel) {
    const uint32_t p = __builtin_amdgcn_perm(0u, w, sel);  // bytes -> [b_hi, 0, b_lo, 0]
    return (p & 0x80008000u) | ((p >> 1) & 0x3F803F80u);
}


// One pass over rows [seg_begin, seg_end) of the shard.
//   NQB: query blocks of 16 (1 or 2).  U: float4 loads per lane per load group (U divides D/16).  A wave keeps
//   kScanSets register sets of U float4: while one group is multiplied, kScanSets - 1 later ones are in flight.
//   kScanThreads per workgroup (one workgroup per CU: LDS holds the queries).
//   SCALE: scores are multiplied by row_scale[row] (a compile-time variant: its load is part of the counted stream).
// Appends are staged per workgroup in LDS (capq entries per query) and flushed once at the end
// with one global atomic per query, so the per-query cursors see ~256 atomics per launch instead
// of one per candidate; entries that do not fit go straight to the global list.
//   F16: the index is stored as f16 (half the HBM bytes); queries are split hi + lo in f16 and
//   multiplied on v_mfma_f32_16x16x32_f16 with f32 accumulation.
//   (F16 == 2: the index is OCP e4m3 with a per-row scale; bytes are widened to f16 in registers.)
constexpr int kScanThreads = 1024;
constexpr int kScanMaxU = 4;  // most loads per lane per group
constexpr int kScanSets = 2;  // register sets of a wave's stream: one group (4 KiB per wave at U = 4) ahead of the MFMAs

//   FILTER: row labels and per-query allow-sets.  Row r is visible to query i iff
//   row_labels[r] < 32 and bit row_labels[r] of query_allow[i] is set.  The label byte of the lane's row is loaded where
//   row_scale is (one byte per lane n at tile change, behind the next tile's first group) and travels with the stream; the
//   lane's 4 NQB allow words stay in registers.  A hidden (query, row) pair is never appended, whatever its score (NaN
//   included) and whatever the threshold (-inf included).  The dense first segment writes every score as before: its
//   selection (k_candidates_select_filtered) reads the labels itself.  FILTER == false is the unfiltered kernel: the two
//   trailing arguments are never read.
template <int NQB, int U, int F16, bool SCALE, bool FILTER = false>
__global__ __launch_bounds__(kScanThreads) void k_cosine_score(
    const float* __restrict__ qfrag, const void* __restrict__ idx, int64_t seg_begin,
    int64_t seg_end, int D, int Q, const float* __restrict__ row_scale,
    const float* __restrict__ tau, float* __restrict__ cand_score, int32_t* __restrict__ cand_id,
    int32_t* __restrict__ cand_cnt, int64_t cap, int dense, int capq, const int32_t* __restrict__ gate,
    const uint8_t* __restrict__ row_labels, const uint32_t* __restrict__ query_allow) {
    if (gate_closed(gate)) return;
    extern __shared__ float4 lds_q[];  // [(D/16)*4][NQB*16] float4, then the append staging area
    constexpr int NQ = NQB * 16;
    constexpr int WAVES = kScanThreads / 64;
    constexpr int NS = kScanSets;
    const int tid = threadIdx.x;
    const int chunks = F16 >= 2 ? D / 64 : (F16 ? D / 32 : D / 16);  // 64-byte pieces of a row
    const int qslots = F16 == 3 ? (D / 8) * NQ  // native fp8: two 1-byte pieces per element, D * NQ * 2 bytes
                                : (D / 16) * 4 * NQ;  // same LDS footprint for the other layouts: D * NQ * 4 bytes
    int* lds_cnt = reinterpret_cast<int*>(lds_q + qslots);          // [32]
    float* lds_sc = reinterpret_cast<float*>(lds_cnt + kQueryBlock);  // [32][capq]
    int* lds_id = reinterpret_cast<int*>(lds_sc + kQueryBlock * capq);  // [32][capq]
    {
        const float4* src = reinterpret_cast<const float4*>(qfrag);
        for (int s = tid; s < qslots; s += kScanThreads) lds_q[s] = src[s];
        if (tid < kQueryBlock) lds_cnt[tid] = 0;
    }
    __syncthreads();

    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // tile and group counters stay scalar
    const int n = lane & 15, g = lane >> 4;
    float tq[NQB][4];
#pragma unroll
    for (int b = 0; b < NQB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qi = b * 16 + 4 * g + r;
            tq[b][r] = qi >= Q ? INFINITY : (dense ? -INFINITY : tau[qi]);
        }

    uint32_t allow[NQB][4];  // FILTER: the allow-sets of this lane's queries (0 for a slot past Q)
    if (FILTER) {
#pragma unroll
        for (int b = 0; b < NQB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qi = b * 16 + 4 * g + r;
                allow[b][r] = qi < Q ? query_allow[qi] : 0u;
            }
    }

    float qs1[NQB][4], qs2[NQB][4];  // native fp8: the two piece scales of this lane's queries
    if (F16 == 3) {
        const float* qscale = reinterpret_cast<const float*>(reinterpret_cast<const char*>(qfrag) + (size_t)D * 2 * NQ);
#pragma unroll
        for (int b = 0; b < NQB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qi = b * 16 + 4 * g + r;
                qs1[b][r] = qscale[qi];
                qs2[b][r] = qscale[kQueryBlock + qi];
            }
    }
    const int64_t seg_rows = seg_end - seg_begin;
    const int tiles = (int)((seg_rows + 15) / 16);  // a shard holds < 2^31 rows: tile indices are 32-bit scalars
    const int groups = chunks / U;
    const float4* lq = lds_q + g * NQ + n;  // + (j*4)*NQ + b*16

    // The wave's work is ONE stream of load groups (U float4 per lane each) that runs across tile boundaries, walked by ONE
    // loop: a step loads the next group of the stream - possibly the first group of the wave's next tile - into one
    // register set, multiplies the group that is in the other, and runs the tile's epilogue when that was the tile's last
    // group.  Two steps with the sets' roles swapped make the loop body, whatever the parity of the group count, so the
    // group in flight across a tile boundary is a loop-carried value of that loop: it is never copied, and every counted
    // vmcnt wait leaves the U newest loads outstanding.  row_scale[row] of a tile is loaded right after the previous
    // tile's epilogue (behind that tile's already issued first group, ahead of every later one), so the epilogue's wait for
    // it leaves at least the newest group outstanding, and the eight threshold tests of a filtered tile end
    // in one ballot: a tile without a candidate (nearly all of them) runs no per-slot code and waits on nothing.
    const int stride = (int)gridDim.x * WAVES;
    const int64_t row_bytes = (int64_t)D * (F16 >= 2 ? 1 : (F16 ? 2 : 4));
    auto tile_ptr = [&](int t) -> const f32x4* {
        const int64_t r = seg_begin + (int64_t)t * 16 + n;
        const int64_t rc = r < seg_end ? r : seg_end - 1;
        return reinterpret_cast<const f32x4*>(static_cast<const char*>(idx) + rc * row_bytes) + g;
    };
    f32x4 acc[NQB], acc_lo[NQB];
    float4 an[NQB];  // f32 rows: the A fragments of the chunk that is multiplied next
    if (F16 == 0) {
#pragma unroll
        for (int b = 0; b < NQB; ++b) an[b] = lq[b * 16];
    }
    auto mul_group = [&](const f32x4 (&x)[U], int gi) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = gi * U + u;
            if (F16 == 3) {  // native fp8 MFMA: index bytes as they are, two e4m3 query pieces, one accumulator each
                typedef uint32_t u32x4n __attribute__((ext_vector_type(4)));
                const u32x4n w = __builtin_bit_cast(u32x4n, x[u]);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const long xb = (long)(((uint64_t)w[2 * m + 1] << 32) | (uint64_t)w[2 * m]);
                    const long* lq8 = reinterpret_cast<const long*>(lds_q) + ((((j * 2 + m) * 4 + g) * 2) * NQ) + n;
#pragma unroll
                    for (int b = 0; b < NQB; ++b) {
                        acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(lq8[b * 16], xb, acc[b], 0, 0, 0);
                        acc_lo[b] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(lq8[NQ + b * 16], xb, acc_lo[b], 0, 0, 0);
                    }
                }
                continue;
            }
            if (F16 == 2) {
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 w = __builtin_bit_cast(u32x4, x[u]);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    u32x4 h;
                    h[0] = fp8x2_to_f16x2_scaled(w[2 * m], 0x010C000Cu);
                    h[1] = fp8x2_to_f16x2_scaled(w[2 * m], 0x030C020Cu);
                    h[2] = fp8x2_to_f16x2_scaled(w[2 * m + 1], 0x010C000Cu);
                    h[3] = fp8x2_to_f16x2_scaled(w[2 * m + 1], 0x030C020Cu);
                    const f16x8 xb = __builtin_bit_cast(f16x8, h);
                    const f16x8* lq16 = reinterpret_cast<const f16x8*>(lds_q) + ((((j * 2 + m) * 4 + g) * 2) * NQ) + n;
#pragma unroll
                    for (int b = 0; b < NQB; ++b) {
                        const f16x8 ah = lq16[b * 16], al = lq16[NQ + b * 16];
                        acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, xb, acc[b], 0, 0, 0);
                        acc_lo[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, xb, acc_lo[b], 0, 0, 0);
                    }
                }
                continue;
            }
            if (F16) {
                const f16x8 xb = __builtin_bit_cast(f16x8, x[u]);
                const f16x8* lq16 = reinterpret_cast<const f16x8*>(lds_q) + ((j * 4 + g) * 2) * NQ + n;
#pragma unroll
                for (int b = 0; b < NQB; ++b) {
                    const f16x8 ah = lq16[b * 16], al = lq16[NQ + b * 16];
                    acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, xb, acc[b], 0, 0, 0);
                    acc_lo[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, xb, acc_lo[b], 0, 0, 0);
                }
                continue;
            }
            // the A fragments of chunk j were read from LDS one chunk ahead (an), the next chunk's are read here, ahead of
            // this chunk's MFMAs; past the tile's last chunk comes chunk 0 of the next tile
            float4 a[NQB];
#pragma unroll
            for (int b = 0; b < NQB; ++b) a[b] = an[b];
            const int jn = j + 1 < chunks ? j + 1 : 0;
#pragma unroll
            for (int b = 0; b < NQB; ++b) an[b] = lq[(jn * 4) * NQ + b * 16];
            __builtin_amdgcn_sched_barrier(0);  // or the reads sink back to just above their first use
            // e outer, query block inner: the two accumulators' chains alternate, so no MFMA waits for the one before
            // it; each accumulator still sees j ascending and, within j, e ascending
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int b = 0; b < NQB; ++b) {
                    const float ab = e == 0 ? a[b].x : (e == 1 ? a[b].y : (e == 2 ? a[b].z : a[b].w));
                    acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(ab, x[u][e], acc[b], 0, 0, 0);
                }
        }
    };

    // the tile's scores against the thresholds; `scale` is row_scale[row] (SCALE only), `label` is row_labels[row] (FILTER only)
    auto epilogue = [&](int64_t row, float scale, uint32_t label) {
        float s[NQB][4];
#pragma unroll
        for (int b = 0; b < NQB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float dot = F16 == 3 ? fmaf(acc_lo[b][r], qs2[b][r], acc[b][r] * qs1[b][r])
                            : (F16 ? fmaf(acc_lo[b][r], 1.0f / kLoScale, acc[b][r]) : acc[b][r]);
                if (F16 == 2) dot *= 256.0f;  // the widened bytes carry value / 256
                s[b][r] = SCALE ? dot * scale : dot;
            }
        if (dense) {  // the first segment: every score is written, nothing is tested
            if (row < seg_end) {
                const int64_t pos = row - seg_begin;
#pragma unroll
                for (int b = 0; b < NQB; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int qi = b * 16 + 4 * g + r;
                        // the id of a dense entry is its position (seg_begin == 0): not stored
                        if (qi < Q) cand_score[qi * cap + pos] = s[b][r];
                    }
            }
            return;
        }
        const uint32_t label_bit = label < 32u ? 1u << label : 0u;  // FILTER: a label >= 32 matches no query
        bool any = false;  // tq is +inf for a query slot past Q; !(s < tq) also lets a NaN score through
#pragma unroll
        for (int b = 0; b < NQB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) any |= !(s[b][r] < tq[b][r]);
        if (FILTER) {  // the filter wins over a threshold of -inf and over a NaN score
            any = false;
#pragma unroll
            for (int b = 0; b < NQB; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) any |= (allow[b][r] & label_bit) != 0u && !(s[b][r] < tq[b][r]);
        }
        any &= row < seg_end;
        if (__ballot(any) == 0) return;
        if (!any) return;  // among them the lanes of a ragged last tile whose row lies past the segment
        // rare from here on.  The slot addresses are derived from an opaque copy of g, so that the compiler computes them
        // here and does not keep sixteen address registers alive through the stream.
        int gq = g;
        asm volatile("" : "+v"(gq));
#pragma unroll
        for (int b = 0; b < NQB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qi = b * 16 + 4 * gq + r;
                if (qi >= Q || !(s[b][r] >= tq[b][r] || s[b][r] != s[b][r])) continue;
                if (FILTER && (allow[b][r] & label_bit) == 0u) continue;
                const int p = atomicAdd(&lds_cnt[qi], 1);
                if (p < capq) {
                    lds_sc[qi * capq + p] = s[b][r];
                    lds_id[qi * capq + p] = (int32_t)row;
                } else {
                    const int32_t pos = atomicAdd(&cand_cnt[qi * kCntStride], 1);
                    cand_score[qi * cap + pos] = s[b][r];
                    cand_id[qi * cap + pos] = (int32_t)row;
                }
            }
    };

    const int t0 = (int)blockIdx.x * WAVES + wave;
    if (t0 < tiles) {
        // load cursor: group gl of tile tl comes next, from lp; multiply cursor: group gm of tile tm
        int tl = t0, tm = t0;
        int gl = 0, gm = 0;
        const f32x4* lp = tile_ptr(tl);
        float scale = 1.0f;
        uint32_t label = 0xFFu;
        auto load_scale = [&]() {
            if (SCALE) {
                const int64_t r = seg_begin + (int64_t)tm * 16 + n;
                scale = row_scale[r < seg_end ? r : seg_end - 1];
            }
            if (FILTER) {
                const int64_t r = seg_begin + (int64_t)tm * 16 + n;
                label = row_labels[r < seg_end ? r : seg_end - 1];
            }
        };
        auto load_next = [&](f32x4 (&x)[U]) {
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = lp[u * 4];
            if (++gl < groups) {
                lp += U * 4;
            } else {  // on to the wave's next tile; past its last one: a harmless re-read of this tile's first group
                gl = 0;
                const int tn = tl + stride;
                tl = tn < tiles ? tn : tl;
                lp = tile_ptr(tl);
            }
        };
        // one step of the stream.  The loop leaves only at its bottom, so a wave may run up to NS - 1 steps past its last
        // tile: they multiply a re-read group and end in no epilogue.  (With an exit after every step the compiler funnels
        // all of them through one latch block, and its wait counts then allow for paths on which a step was skipped.)
        auto step = [&](const f32x4 (&cur)[U], f32x4 (&nxt)[U]) {
            load_next(nxt);
            __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of the MFMAs it overlaps
            mul_group(cur, gm);
            __builtin_amdgcn_sched_barrier(0);
            if (++gm < groups) return;
            if (tm < tiles) epilogue(seg_begin + (int64_t)tm * 16 + n, scale, label);
            gm = 0;
            tm += stride;
#pragma unroll
            for (int b = 0; b < NQB; ++b) acc[b] = acc_lo[b] = (f32x4){0.f, 0.f, 0.f, 0.f};
            load_scale();
        };
        f32x4 x[NS][U];
#pragma unroll
        for (int b = 0; b < NQB; ++b) acc[b] = acc_lo[b] = (f32x4){0.f, 0.f, 0.f, 0.f};
        load_scale();
#pragma unroll
        for (int s = 0; s < NS - 1; ++s) load_next(x[s]);
        do {
#pragma unroll
            for (int s = 0; s < NS; ++s) step(x[s], x[(s + NS - 1) % NS]);
        } while (tm < tiles);
    }

    if (!dense && capq > 0) {
        __syncthreads();
        for (int qi = wave; qi < Q; qi += WAVES) {
            int cnt = lds_cnt[qi];
            cnt = cnt < capq ? cnt : capq;
            if (cnt <= 0) continue;
            int base = 0;
            if (lane == 0) base = atomicAdd(&cand_cnt[qi * kCntStride], cnt);
            base = __shfl(base, 0, 64);
            for (int e = lane; e < cnt; e += 64) {
                cand_score[qi * cap + base + e] = lds_sc[qi * capq + e];
                cand_id[qi * cap + base + e] = lds_id[qi * capq + e];
            }
        }
    }
}

// The k output slots of query qi from sh.keys[0..m): (score, row_id_base + id), then (-inf, -1).  A key 0 inside [0, m)
// is padding too; no real entry encodes to 0 (row ids are < 2^31 - 1, so the low word 0xFFFFFFFF - id is never 0).
__device__ inline void write_topk(const SelectShared& sh, int m, int qi, int k, int64_t row_id_base,
                                  float* __restrict__ out_score, int64_t* __restrict__ out_index) {
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        const uint64_t key = i < m ? sh.keys[i] : 0ull;
        out_score[(int64_t)qi * k + i] = key != 0ull ? key_score(key) : -INFINITY;
        out_index[(int64_t)qi * k + i] = key != 0ull ? row_id_base + (int64_t)key_index(key) : -1;
    }
}

// One workgroup per query: exact top-k of its candidate list, written back sorted to the head of
// the list; raises tau to the k-th score.  The last call of a batch also writes the outputs.
//   FILTER (k_candidates_select_filtered): the dense first segment holds a score for EVERY (query, row) pair, so its
//   selection reads the row's label beside the score and turns a hidden entry into a key below every real one: high word 0
//   (the smallest real high word is that of -inf, 0x007FFFFF), low word as for a real key, so the keys stay distinct and
//   non-zero as block_topk requires.  Sorted, the real keys come first; only those are written back, counted and allowed to
//   raise tau (k sorted keys are not enough: k REAL keys are needed).  Later segments append visible pairs only, so their
//   lists hold nothing but real keys.  FILTER == false compiles to the unfiltered kernel.
template <bool FILTER>
__device__ __forceinline__ void candidates_select_pass(
    float* __restrict__ cand_score, int32_t* __restrict__ cand_id, int32_t* __restrict__ cand_cnt,
    float* __restrict__ tau, int64_t cap, int k, int64_t dense_count, int final_pass,
    int64_t row_id_base, float* __restrict__ out_score, int64_t* __restrict__ out_index,
    const uint8_t* __restrict__ row_labels, const uint32_t* __restrict__ query_allow) {
    __shared__ SelectShared sh;
    const int qi = blockIdx.x;
    const float* cs = cand_score + qi * cap;
    const int32_t* ci = cand_id + qi * cap;
    const int64_t cnt = dense_count >= 0 ? dense_count : (int64_t)cand_cnt[qi * kCntStride];
    // A workgroup pulls its list through ONE CU's memory pipeline (~30 GB/s from HBM), several passes over it: the
    // 65 536 (score, id) pairs of a dense first segment are 1.5 - 2 MB of reads, most of that selection's 75 us.  In the
    // dense segment entry i IS row i of the shard (the segment starts at row 0), so its ids are never read.
    const bool dense = dense_count >= 0;
    const uint32_t allow = FILTER ? query_allow[qi] : 0u;
    auto load = [&](int64_t i) -> uint64_t {
        const uint64_t key = make_key(cs[i], dense ? (uint32_t)i : (uint32_t)ci[i]);
        if (FILTER) {
            // dense entry i is row i of the shard.  The label load is unconditional (row 0 for a later list, whose entries are
            // all visible), like the loads of block_topk's radix loops: no branch between two keys' loads
            const uint32_t label = row_labels[dense ? i : 0];
            const bool hidden = dense && (label >= 32u || ((allow >> label) & 1u) == 0u);
            return hidden ? key & 0xFFFFFFFFull : key;  // hidden: below every real key
        }
        return key;
    };
    int m = block_topk(sh, load, cnt, k);
    // block_topk ends on a barrier: every read of the old list is done before it is overwritten.
    if (FILTER && dense) {  // keep the real keys of the m sorted ones: they come first
        if (threadIdx.x == 0) sh.scalar[3] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += blockDim.x)
            if ((sh.keys[i] >> 32) != 0ull && (i + 1 == m || (sh.keys[i + 1] >> 32) == 0ull)) sh.scalar[3] = (uint32_t)(i + 1);
        __syncthreads();
        m = (int)sh.scalar[3];
    }
    for (int i = threadIdx.x; i < m; i += blockDim.x) {
        const uint64_t key = sh.keys[i];
        cand_score[qi * cap + i] = key_score(key);
        cand_id[qi * cap + i] = (int32_t)key_index(key);
    }
    if (threadIdx.x == 0) {
        cand_cnt[qi * kCntStride] = m;
        if (m == k) tau[qi] = key_score(sh.keys[k - 1]);
    }
    if (final_pass) write_topk(sh, m, qi, k, row_id_base, out_score, out_index);
}

__global__ __launch_bounds__(kSelectThreads) void k_candidates_select(
    float* __restrict__ cand_score, int32_t* __restrict__ cand_id, int32_t* __restrict__ cand_cnt,
    float* __restrict__ tau, int64_t cap, int k, int64_t dense_count, int final_pass,
    int64_t row_id_base, float* __restrict__ out_score, int64_t* __restrict__ out_index,
    const int32_t* __restrict__ gate) {
    if (gate_closed(gate)) return;
    candidates_select_pass<false>(cand_score, cand_id, cand_cnt, tau, cap, k, dense_count, final_pass, row_id_base, out_score,
                                  out_index, nullptr, nullptr);
}

__global__ __launch_bounds__(kSelectThreads) void k_candidates_select_filtered(
    float* __restrict__ cand_score, int32_t* __restrict__ cand_id, int32_t* __restrict__ cand_cnt,
    float* __restrict__ tau, int64_t cap, int k, int64_t dense_count, int final_pass,
    int64_t row_id_base, float* __restrict__ out_score, int64_t* __restrict__ out_index,
    const int32_t* __restrict__ gate, const uint8_t* __restrict__ row_labels, const uint32_t* __restrict__ query_allow) {
    if (gate_closed(gate)) return;
    candidates_select_pass<true>(cand_score, cand_id, cand_cnt, tau, cap, k, dense_count, final_pass, row_id_base, out_score,
                                 out_index, row_labels, query_allow);
}

struct WsLayout {
    size_t qfrag_off, tau_off, cnt_off, score_off, id_off, total;
    int64_t cap;
};

static WsLayout ws_layout(int D, int k, int64_t seg_max) {
    WsLayout w;
    Bump m;
    w.cap = seg_max + k;
    w.qfrag_off = m.take((size_t)D * kQueryBlock * sizeof(float));
    w.tau_off = m.take(kQueryBlock * sizeof(float));
    w.cnt_off = m.take((size_t)kQueryBlock * kCntStride * sizeof(int32_t));
    w.score_off = m.take((size_t)kQueryBlock * w.cap * sizeof(float));
    w.id_off = m.take((size_t)kQueryBlock * w.cap * sizeof(int32_t));
    w.total = m.total;
    return w;
}

static int64_t clamp_seg(int64_t N, int64_t want) {
    int64_t s = N < want ? N : want;
    return s < 1 ? 1 : s;
}

struct ScoreArgs {
    int grid;
    size_t lds;
    hipStream_t st;
    const float* qfrag;
    const void* idx;
    int64_t b, e;
    int D, Q;
    const float* row_scale;
    const float* tau;
    float* cs;
    int32_t* ci;
    int32_t* cc;
    int64_t cap;
    int dense, capq;
    const int32_t* gate;
    const uint8_t* row_labels;    // both null: the unfiltered kernels
    const uint32_t* query_allow;  // the allow-sets of this pass's queries
};

template <int NQB, int U, int KIND, bool SCALE, bool FILTER>
static int launch_score(const ScoreArgs& a) {
    static thread_local bool attr_set = false;
    if (!attr_set) {
        EVI_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cosine_score<NQB, U, KIND, SCALE, FILTER>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
    }
    // gated launches (the fallback of a proof-carrying path) stay out of the timing accounts
    launch_timed(a.gate ? kUntimed : kTimeCosineScore, k_cosine_score<NQB, U, KIND, SCALE, FILTER>, dim3(a.grid),
                 dim3(kScanThreads), a.lds, a.st, a.qfrag, a.idx, a.b, a.e, a.D, a.Q, a.row_scale, a.tau, a.cs, a.ci, a.cc, a.cap,
                 a.dense, a.capq, a.gate, a.row_labels, a.query_allow);
    EVI_LAUNCH_CHECK();
    return EVI_OK;
}

// the filter is a compile-time variant like row_scale: a call without labels launches the FILTER = false instantiation
template <int NQB, int U, int KIND, bool SCALE>
static int launch_score_filter(const ScoreArgs& a) {
    return a.row_labels ? launch_score<NQB, U, KIND, SCALE, true>(a) : launch_score<NQB, U, KIND, SCALE, false>(a);
}

// row_scale is a compile-time variant (its load is part of the counted stream).  An e4m3 index always has one: the
// SCALE kernel reads row_scale without a null test, and cosine_topk_impl refuses an e4m3 index without it (EVI_REQUIRE)
// before anything is launched, so the unscaled form of those kinds is never instantiated.
template <int NQB, int U, int KIND>
static int launch_score_scale(const ScoreArgs& a) {
    if constexpr (KIND >= kIdxFp8Widen) {
        return launch_score_filter<NQB, U, KIND, true>(a);
    } else {
        return a.row_scale ? launch_score_filter<NQB, U, KIND, true>(a) : launch_score_filter<NQB, U, KIND, false>(a);
    }
}

template <int NQB, int KIND>
static int launch_score_u(int U, const ScoreArgs& a) {
    switch (U) {
        case 4: return launch_score_scale<NQB, 4, KIND>(a);
        case 2: return launch_score_scale<NQB, 2, KIND>(a);
        default: return launch_score_scale<NQB, 1, KIND>(a);
    }
}

static int launch_score_kind(IndexKind kind, int nqb, int U, const ScoreArgs& a) {
    switch (kind * 2 + (nqb - 1)) {
        case kIdxF32 * 2: return launch_score_u<1, kIdxF32>(U, a);
        case kIdxF32 * 2 + 1: return launch_score_u<2, kIdxF32>(U, a);
        case kIdxF16 * 2: return launch_score_u<1, kIdxF16>(U, a);
        case kIdxF16 * 2 + 1: return launch_score_u<2, kIdxF16>(U, a);
        case kIdxFp8Widen * 2: return launch_score_u<1, kIdxFp8Widen>(U, a);
        case kIdxFp8Widen * 2 + 1: return launch_score_u<2, kIdxFp8Widen>(U, a);
        case kIdxFp8Mfma * 2: return launch_score_u<1, kIdxFp8Mfma>(U, a);
        default: return launch_score_u<2, kIdxFp8Mfma>(U, a);
    }
}

// the batch's query fragments in the layout `kind` multiplies (also resets the batch's selection state)
static void launch_query_fragments(IndexKind kind, hipStream_t st, const float* q, int Q, int D, int nq_pad, float* qfrag,
                                   float* tau, int32_t* cnt, const int32_t* gate) {
    f16x8* qfrag16 = reinterpret_cast<f16x8*>(qfrag);
    switch (kind) {
        case kIdxFp8Mfma:  // one workgroup per query slot
            hipLaunchKernelGGL(k_query_fragments_fp8n, dim3(nq_pad), dim3(256), 0, st, q, Q, D, nq_pad,
                               reinterpret_cast<uint64_t*>(qfrag), tau, cnt, gate);
            break;
        case kIdxFp8Widen:
            hipLaunchKernelGGL(k_query_fragments_fp8, dim3(32), dim3(256), 0, st, q, Q, D, nq_pad, qfrag16, tau, cnt, gate);
            break;
        case kIdxF16:
            hipLaunchKernelGGL(k_query_fragments_f16, dim3(32), dim3(256), 0, st, q, Q, D, nq_pad, qfrag16, tau, cnt, gate);
            break;
        default:
            hipLaunchKernelGGL(k_query_fragments, dim3(32), dim3(256), 0, st, q, Q, D, nq_pad, qfrag, tau, cnt, gate);
    }
}

// Segment schedule knobs (tuning only; results do not depend on them):
//   EVI_SCAN_FIRST   rows of the dense first segment, [4096, 65536] (default 65536)
//   EVI_SCAN_GROWTH  next segment = growth x rows scanned so far, [2, 256] (default 16)
struct SegmentSchedule {
    int64_t first, growth;
};
static SegmentSchedule segment_schedule() {
    static SegmentSchedule s{0, 0};
    if (s.first == 0) {
        int64_t first = kFirstSegment, growth = kSegmentGrowth;
        if (const char* e = getenv("EVI_SCAN_FIRST")) first = atoll(e);
        if (const char* e = getenv("EVI_SCAN_GROWTH")) growth = atoll(e);
        first = first < 4096 ? 4096 : (first > kFirstSegment ? kFirstSegment : first);
        first = (first + 15) / 16 * 16;
        growth = growth < 2 ? 2 : (growth > 256 ? 256 : growth);
        s = SegmentSchedule{first, growth};
    }
    return s;
}

static int device_cu_count() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            cus = prop.multiProcessorCount;
        if (cus <= 0) cus = 256;
    }
    return cus;
}

}  // namespace evi

using namespace evi;

extern "C" size_t evi_cosine_topk_workspace_bytes(int Q, int64_t N, int D, int k) {
    (void)Q;
    if (D <= 0 || k <= 0 || N < 0) return 0;
    return ws_layout(D, k, clamp_seg(N, kMaxSegmentDefault)).total;
}

extern "C" size_t evi_cosine_topk_min_workspace_bytes(int Q, int64_t N, int D, int k) {
    (void)Q;
    if (D <= 0 || k <= 0 || N < 0) return 0;
    return ws_layout(D, k, clamp_seg(N, kFirstSegment)).total;
}

static int cosine_topk_impl(const float* q, int Q, const void* idx, IndexKind kind, int64_t N, int D,
                            const float* row_scale, int k, int64_t row_id_base, float* out_score,
                            int64_t* out_index, void* workspace, size_t workspace_bytes, void* stream,
                            const int32_t* gate = nullptr, const uint8_t* row_labels = nullptr,
                            const uint32_t* query_allow = nullptr) {
    EVI_REQUIRE((row_labels == nullptr) == (query_allow == nullptr), "evi_cosine_topk: row_labels and query_allow go together");
    EVI_REQUIRE(Q >= 1, "evi_cosine_topk: Q must be >= 1, got %d", Q);
    EVI_REQUIRE(N >= 0, "evi_cosine_topk: N must be >= 0, got %lld", (long long)N);
    EVI_REQUIRE(N < (int64_t)0x7FFFFFFF, "evi_cosine_topk: a shard holds at most 2^31-1 rows, got %lld",
                (long long)N);
    EVI_REQUIRE(k >= 1 && k <= EVI_TOPK_MAX_K, "evi_cosine_topk: k must be in [1, %d], got %d",
                EVI_TOPK_MAX_K, k);
    EVI_REQUIRE(q && out_score && out_index, "evi_cosine_topk: null q/out pointer");
    EVI_REQUIRE(N == 0 || idx, "evi_cosine_topk: null idx with N > 0");
    if (D < 16 || D % 16 != 0 || D > 1280)
        return fail(EVI_ERR_UNSUPPORTED,
                    "evi_cosine_topk: D must be a multiple of 16 in [16, 1280], got %d", D);
    if (kind == kIdxF16 && D % 32 != 0)
        return fail(EVI_ERR_UNSUPPORTED, "evi_cosine_topk_f16: D must be a multiple of 32, got %d", D);
    if (kind >= kIdxFp8Widen && D % 64 != 0)
        return fail(EVI_ERR_UNSUPPORTED, "evi_cosine_topk_fp8: D must be a multiple of 64, got %d", D);
    EVI_REQUIRE(kind < kIdxFp8Widen || row_scale || N == 0, "evi_cosine_topk_fp8: row_scale (the per-row dequantisation scale) is required");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    const size_t min_ws = evi_cosine_topk_min_workspace_bytes(Q, N, D, k);
    EVI_REQUIRE(workspace != nullptr, "evi_cosine_topk: null workspace");
    if (workspace_bytes < min_ws)
        return fail(EVI_ERR_NOMEM, "evi_cosine_topk: workspace %zu B < minimum %zu B", workspace_bytes,
                    min_ws);
    // Largest segment the workspace can hold (halve until it fits).
    int64_t seg_max = clamp_seg(N, kMaxSegmentDefault);
    while (seg_max > kFirstSegment && ws_layout(D, k, seg_max).total > workspace_bytes) seg_max >>= 1;
    if (seg_max < clamp_seg(N, kFirstSegment)) seg_max = clamp_seg(N, kFirstSegment);
    const WsLayout w = ws_layout(D, k, seg_max);
    char* base = static_cast<char*>(workspace);
    float* qfrag = reinterpret_cast<float*>(base + w.qfrag_off);
    float* tau = reinterpret_cast<float*>(base + w.tau_off);
    int32_t* cnt = reinterpret_cast<int32_t*>(base + w.cnt_off);
    float* cs = reinterpret_cast<float*>(base + w.score_off);
    int32_t* ci = reinterpret_cast<int32_t*>(base + w.id_off);

    const int chunks = index_chunks(kind, D);
    // loads per lane per group: the largest U <= kScanMaxU that leaves an even number of groups, else the largest U that
    // divides the row.  The stream loop is copy-free for either parity, so the evenness no longer buys anything by itself;
    // the rule is kept because every measured leg (D = 768: U = 4 for f32 / f16, U = 2 for e4m3) was measured with it.
    int U = 1;
    for (int cand = kScanMaxU; cand >= 1; cand >>= 1)
        if (chunks % (2 * cand) == 0) { U = cand; break; }
    if (U == 1 && chunks % 2 != 0)
        for (int cand = kScanMaxU; cand >= 1; cand >>= 1)
            if (chunks % cand == 0) { U = cand; break; }
    const int cus = device_cu_count();
    const int waves_per_block = kScanThreads / 64;

    // 32 queries per pass when their fragments (+ the append counters) fit the 160 KiB of LDS, else 16: at D = 1280 the
    // f32 / f16 / widened-fp8 fragments of 32 queries are exactly 160 KiB and leave no room for the counters
    const int qblock = query_frag_bytes(kind, D, kQueryBlock) + kQueryBlock * sizeof(int) > 160 * 1024 ? 16 : kQueryBlock;
    for (int q0 = 0; q0 < Q; q0 += qblock) {
        const int qn = (Q - q0) < qblock ? (Q - q0) : qblock;
        const int nqb = qn <= 16 ? 1 : 2;
        const int nq_pad = nqb * 16;
        float* o_score = out_score + (int64_t)q0 * k;
        int64_t* o_index = out_index + (int64_t)q0 * k;

        launch_query_fragments(kind, st, q + (int64_t)q0 * D, qn, D, nq_pad, qfrag, tau, cnt, gate);
        EVI_LAUNCH_CHECK();

        if (N == 0) {
            hipLaunchKernelGGL(k_candidates_select, dim3(qn), dim3(kSelectThreads), 0, st, cs, ci, cnt,
                               tau, w.cap, k, (int64_t)0, 1, row_id_base, o_score, o_index, gate);
            EVI_LAUNCH_CHECK();
            continue;
        }
        const size_t lds_q_bytes = query_frag_bytes(kind, D, nq_pad);
        // staging entries per query: whatever LDS is left, at most 64
        const int64_t lds_left = (int64_t)160 * 1024 - (int64_t)lds_q_bytes - (int64_t)(kQueryBlock * sizeof(int));
        int capq = lds_left > 0 ? (int)(lds_left / (kQueryBlock * 8)) : 0;
        capq = capq > 64 ? 64 : capq;
        const size_t lds = lds_q_bytes + kQueryBlock * sizeof(int) + (size_t)kQueryBlock * capq * 8;
        int64_t begin = 0;
        const SegmentSchedule sched = segment_schedule();
        int64_t seg = clamp_seg(N, sched.first);
        bool first = true;
        while (begin < N) {
            int64_t end = begin + seg;
            if (end > N) end = N;
            const int64_t tiles = (end - begin + 15) / 16;
            int64_t want = (tiles + waves_per_block - 1) / waves_per_block;
            const int grid = (int)(want < cus ? want : cus);
            const uint32_t* allow = query_allow ? query_allow + q0 : nullptr;
            const ScoreArgs sa{grid, lds, st, qfrag, idx, begin, end, D, qn, row_scale, tau,
                               cs, ci, cnt, w.cap, first ? 1 : 0, capq, gate, row_labels, allow};
            const int rc = launch_score_kind(kind, nqb, U, sa);
            if (rc != EVI_OK) return rc;
            const int final_pass = end >= N ? 1 : 0;
            if (row_labels)
                launch_timed(gate ? kUntimed : kTimeSelect, k_candidates_select_filtered, dim3(qn), dim3(kSelectThreads), 0, st, cs,
                             ci, cnt, tau, w.cap, k, first ? (end - begin) : (int64_t)-1, final_pass, row_id_base, o_score, o_index,
                             gate, row_labels, allow);
            else
                launch_timed(gate ? kUntimed : kTimeSelect, k_candidates_select, dim3(qn), dim3(kSelectThreads), 0, st, cs, ci, cnt,
                             tau, w.cap, k, first ? (end - begin) : (int64_t)-1, final_pass, row_id_base, o_score, o_index, gate);
            EVI_LAUNCH_CHECK();
            begin = end;
            first = false;
            int64_t next = begin * sched.growth;
            seg = next < seg_max ? next : seg_max;
            if (seg < 1) seg = 1;
        }
    }
    return EVI_OK;
}

extern "C" int evi_cosine_topk(const float* q, int Q, const float* idx, int64_t N, int D,
                               const float* row_scale, int k, int64_t row_id_base, float* out_score,
                               int64_t* out_index, void* workspace, size_t workspace_bytes,
                               void* stream) {
    return cosine_topk_impl(q, Q, idx, kIdxF32, N, D, row_scale, k, row_id_base, out_score, out_index, workspace,
                            workspace_bytes, stream);
}

extern "C" int evi_cosine_topk_f16(const float* q, int Q, const void* idx_f16, int64_t N, int D,
                                   const float* row_scale, int k, int64_t row_id_base, float* out_score,
                                   int64_t* out_index, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    return cosine_topk_impl(q, Q, idx_f16, kIdxF16, N, D, row_scale, k, row_id_base, out_score, out_index, workspace,
                            workspace_bytes, stream);
}

extern "C" int evi_cosine_topk_fp8(const float* q, int Q, const void* idx_fp8, int64_t N, int D,
                                   const float* row_scale, int k, int64_t row_id_base, float* out_score,
                                   int64_t* out_index, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    return cosine_topk_impl(q, Q, idx_fp8, kIdxFp8Widen, N, D, row_scale, k, row_id_base, out_score, out_index, workspace,
                            workspace_bytes, stream);
}

extern "C" int evi_cosine_topk_fp8_mfma(const float* q, int Q, const void* idx_fp8, int64_t N, int D,
                                        const float* row_scale, int k, int64_t row_id_base, float* out_score,
                                        int64_t* out_index, void* workspace, size_t workspace_bytes, void* stream) {
    return cosine_topk_impl(q, Q, idx_fp8, kIdxFp8Mfma, N, D, row_scale, k, row_id_base, out_score, out_index, workspace,
                            workspace_bytes, stream);
}

extern "C" int evi_cosine_topk_filtered(const float* q, int Q, const void* idx, int kind, int64_t N, int D,
                                        const float* row_scale, const uint8_t* row_labels, const uint32_t* query_allow, int k,
                                        int64_t row_id_base, float* out_score, int64_t* out_index, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    EVI_REQUIRE(kind >= kIdxF32 && kind <= kIdxFp8Mfma, "evi_cosine_topk_filtered: kind must be 0 (f32), 1 (f16), 2 (e4m3 widened) "
                "or 3 (e4m3 native MFMA), got %d", kind);
    EVI_REQUIRE(row_labels && query_allow, "evi_cosine_topk_filtered: null row_labels / query_allow");
    return cosine_topk_impl(q, Q, idx, (IndexKind)kind, N, D, row_scale, k, row_id_base, out_score, out_index, workspace,
                            workspace_bytes, stream, nullptr, row_labels, query_allow);
}

// =====================================================================================================
// Many queries (Q in the hundreds): GEMM-shaped, still exact.
//
// The scan above holds 32 queries in LDS and streams the index once per 32 queries: at Q = 512 that is
// 16 passes, bound by the f32 MFMA rate.  Here the scores of ALL queries against a slab of index rows
// are formed as one split-bf16 GEMM (bf16 MFMA, f32 accumulate: |error| <= 2.5e-4 * |q| |x|, see
// kApproxEps) — approximate, so they only SELECT: every query keeps its kk = k + reserve best rows by
// approximate score, and the call succeeds only if the k-th and the kk-th approximate scores are more
// than 2 eps apart, which proves that the true top-k (by the scan's own f32 arithmetic) is inside the
// kk kept rows.  Those kk rows are then re-scored with exactly the scan's instruction sequence
// (v_mfma_f32_16x16x4_f32 over d in the same order), and the final top-k is taken on those scores: ids
// and scores are bit-identical to evi_cosine_topk.  When the gap test fails (heavy ties, adversarial
// data) or a candidate list overflows, *status is set and the caller runs the scan instead.
// =====================================================================================================
namespace evi {

constexpr float kApproxEps = 2.5e-4f;        // |gemm score - scan score| <= kApproxEps * |q| for unit-norm rows:
                                             // bf16 hi/lo split 2^-16 + 2^-18, 2304 f32 accumulations x 2^-24,
                                             // plus the scan's own 768 x 2^-24
constexpr float kApproxEps1 = 4.2e-3f;       // single-product selection: both operands rounded to bf16 (2 x 2^-9 + 2^-18
                                             // relative per product), 768 accumulations, plus the scan's own error
// e4m3 index (evi_cosine_topk_gemm_fp8), both scan variants: |selection score - scan score| <= kApproxEpsFp8Unit * |q| * |x|
// for the STORED row x (codes x row_scale), D <= 1280, every f32 accumulation charged 2^-23 (truncating adders assumed,
// as for kShadowEps).  Term by term, relative to |q| |x| (Cauchy-Schwarz on each sum):
//   index side of the selection product                       0        an e4m3 code is exactly a bf16 value
//   query of the selection, widening variant                  2^-16    f32 query as bf16 hi + lo, (2^-8)^2
//   query of the scan, widening variant                       2^-22    f32 query as f16 hi + lo, (2^-11)^2
//   query, native variant                                     0        selection and scan multiply the SAME two e4m3
//                                                                      pieces; the power-of-two piece scales commute
//                                                                      with every rounding
//   selection GEMM: 2 products x D into one accumulator       2560 x 2^-23
//   scan: D products into each of two accumulators            1280 x 2^-23   (the lo accumulator is <= 2^-8 of the hi one)
//   combining fma of the scan, row_scale multiply on each side   3 x 2^-23
//   sum: (2560 + 1280 + 3) x 2^-23 + 2^-16 + 2^-22 = 4.58e-4 + 1.55e-5 = 4.74e-4
// The widening variant's query terms are relative to each element, which f16 grants only to queries of ordinary size:
// the gap test refuses a query with |q| outside [1/4, 4] (as the two-stage path does) and the scan takes the batch.
// Stored e4m3 rows are not unit norm: rounding to 4 significant bits moves each element by <= 2^-4 of itself, so a unit
// row is stored with |x| <= 1 + 2^-4.  That is the tolerance the caller's norm check applies (kFp8RowNormMax); the proof
// uses the product of the two.
constexpr float kApproxEpsFp8Unit = 4.8e-4f;
constexpr float kFp8RowNormMax = 1.0625f;
constexpr float kApproxEpsFp8 = kApproxEpsFp8Unit * kFp8RowNormMax;  // 5.1e-4
constexpr int kGemmTopkCap = 16384;          // candidate slots per query between two selections
constexpr int64_t kGemmFirstRows = 4096;     // first slab: every row is a candidate (4096 <= cap)
constexpr int64_t kGemmSlabRows = 1 << 21;   // rows per GEMM launch between two selections (bounds the appends)
constexpr int kGemmGrowth = 8;

// candidates kept per query: the coarser the selection scores, the more rows can hide inside 2 eps of the k-th
static int gemm_topk_reserve(int k, int single = 0) {
    if (single) return k + (k > 1024 ? k : 1024);
    int r = k / 2 > 256 ? k / 2 : 256;
    return k + r;
}

__global__ void k_gt_init(float* tau, int32_t* cnt, int Q, int32_t* status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Q) {
        tau[i] = -INFINITY;
        cnt[i * kCntStride] = 0;
    }
    if (i == 0) *status = 0;
}

// scores [rows, Q] (row-major) of slab rows [row0, row0 + rows): append (score * row_scale, row) to the list of
// every query whose current threshold it reaches.  FILTER: only where the row is visible to the query (row_labels[row] < 32
// and bit row_labels[row] of query_allow[query] set) — a hidden pair is never appended, NaN score or not; FILTER == false
// is the unfiltered kernel and reads neither array.
template <bool FILTER>
__global__ __launch_bounds__(256) void k_gt_filter(const float* __restrict__ scores, int64_t rows, int Q, int64_t row0,
                                                   const float* __restrict__ row_scale, const float* __restrict__ tau,
                                                   float* __restrict__ cand_score, int32_t* __restrict__ cand_id,
                                                   int32_t* __restrict__ cand_cnt, int32_t* __restrict__ status,
                                                   const uint8_t* __restrict__ row_labels,
                                                   const uint32_t* __restrict__ query_allow) {
    const int64_t total = rows * Q;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / Q;
        const int qi = (int)(i - r * Q);
        float s = scores[i];
        if (row_scale) s *= row_scale[row0 + r];
        if (s >= tau[qi] || s != s) {
            if (FILTER) {
                const uint32_t label = row_labels[row0 + r];
                if (label >= 32u || ((query_allow[qi] >> label) & 1u) == 0u) continue;
            }
            const int32_t pos = atomicAdd(&cand_cnt[qi * kCntStride], 1);
            if (pos < kGemmTopkCap) {
                cand_score[(int64_t)qi * kGemmTopkCap + pos] = s;
                cand_id[(int64_t)qi * kGemmTopkCap + pos] = (int32_t)(row0 + r);
            } else {
                atomicOr(status, 2);  // list full: the caller falls back to the scan
            }
        }
    }
}

// after an overflowing slab the cursor may exceed the capacity: clamp before the selection reads the list
__global__ void k_gt_clamp(int32_t* cnt, int Q) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Q && cnt[i * kCntStride] > kGemmTopkCap) cnt[i * kCntStride] = kGemmTopkCap;
}

// The proof both fast paths share: with kk rows kept by approximate score, the true top-k is among them when
// approx[k-1] - approx[kk-1] > 2 eps |q|.  wave_sumsq is |q|^2 in ONE fixed order (lane-strided fmaf, xor butterfly), to
// all 64 lanes; which lists are tested and which flags a failure raises is the caller's policy.
__device__ inline float wave_sumsq(const float* __restrict__ q, int D, int lane) {
    float ss = 0.f;
    for (int d = lane; d < D; d += 64) ss = fmaf(q[d], q[d], ss);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    return ss;
}
__device__ inline bool gap_fails(float gap, float eps, float ss) { return !(gap > 2.0f * eps * sqrtf(ss)); }  // NaN fails too

// q_norm_guard: the bound also needs |q| in [1/4, 4] (an f16 hi / lo split of the query is part of it)
__global__ void k_gt_gap(const float* __restrict__ q, int Q, int D, const float* __restrict__ cand_score,
                         const int32_t* __restrict__ cand_cnt, int k, int kk, float eps, int q_norm_guard,
                         int32_t* __restrict__ status) {
    const int qi = blockIdx.x;
    const int lane = threadIdx.x;  // one wave
    const float ss = wave_sumsq(q + (int64_t)qi * D, D, lane);
    if (lane == 0) {
        const int m = cand_cnt[qi * kCntStride];
        if (m >= kk) {
            const float* s = cand_score + (int64_t)qi * kGemmTopkCap;
            const bool norm_ok = !q_norm_guard || (ss >= 0.0625f && ss <= 16.0f);
            if (gap_fails(s[k - 1] - s[kk - 1], eps, ss) || !norm_ok) atomicOr(status, 1);
        }  // m < kk: every row of the index (with a row filter: every row visible to this query) is in the list
    }
}

// Exact re-scoring of candidate rows with the scan's arithmetic: the score of (query, row) is the chain
//   for j = 0 .. D/16 - 1, e = 0 .. 3:  acc = mfma_16x16x4(a = q[16 j + 4 g + e], b = x[16 j + 4 g + e], acc)
// over lane groups g = 0..3 — exactly what k_cosine_score feeds for that pair (an MFMA output element depends
// only on its own row of A and column of B).  One wave per (query, 16 candidates): the query sits in row 0 of A, the
// candidates (lane n = l & 15 brings row x) in the 16 columns of B; D[row 0][col n] is returned to the lanes with g == 0.
// This chain IS the bit-exactness contract of the GEMM-shaped and two-stage paths with the scan.
__device__ inline float rescore_chain(const float* __restrict__ q, const float* __restrict__ x_row, int D, int n, int g) {
    const f32x4* xp = reinterpret_cast<const f32x4*>(x_row) + g;
    const f32x4* qp = reinterpret_cast<const f32x4*>(q) + g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // eight 64-byte pieces of the row in flight per lane group: the rows are scattered over the index, so a loop that
    // waits for each piece is bound by the HBM latency (48 round trips at D = 768); the MFMA order is unchanged
    constexpr int PF = 8;
    const int J = D / 16;
    for (int j0 = 0; j0 < J; j0 += PF) {
        f32x4 x[PF], a[PF];
#pragma unroll
        for (int u = 0; u < PF; ++u) {  // unconditional loads (a piece past the end re-reads the last one): a bounds
            const int j = j0 + u < J ? j0 + u : J - 1;  // branch here would make the compiler wait for each load in turn
            x[u] = xp[j * 4];
            a[u] = n == 0 ? qp[j * 4] : zero;
        }
#pragma unroll
        for (int u = 0; u < PF; ++u)
            if (j0 + u < J) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][e], x[u][e], acc, 0, 0, 0);
            }
    }
    return acc[0];
}

// The same for an f16-stored index: the scan multiplies the f16 rows with the query split hi + lo (lo scaled by
// kLoScale) on v_mfma_f32_16x16x32_f16 into two accumulators, chunk by chunk of 32 dims, and combines them as
// fma(acc_lo, 1 / kLoScale, acc).
__device__ inline float rescore_chain(const float* __restrict__ q, const _Float16* __restrict__ x_row, int D, int n, int g) {
    const f16x8* xp = reinterpret_cast<const f16x8*>(x_row) + g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc_lo = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < D / 32; ++j) {
        const f16x8 x = xp[j * 4];
        f16x8 ah, al;
#pragma unroll
        for (int e = 0; e < 8; ++e) {  // the split of k_query_fragments_f16
            const float v = n == 0 ? q[32 * j + 8 * g + e] : 0.f;
            const _Float16 h = (_Float16)v;
            ah[e] = h;
            al[e] = (_Float16)((v - (float)h) * kLoScale);
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, x, acc, 0, 0, 0);
        acc_lo = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, x, acc_lo, 0, 0, 0);
    }
    return fmaf(acc_lo[0], 1.0f / kLoScale, acc[0]);
}

// An e4m3 index has two scan variants with different arithmetic, so a row pointer carries the variant as its type (one
// byte per element either way).
struct Fp8WidenRow { uint8_t code; };  // kIdxFp8Widen
struct Fp8MfmaRow { uint8_t code; };   // kIdxFp8Mfma

// kIdxFp8Widen: per 64-byte piece j lane group g owns bytes 16 g .. + 15, widened to f16 (value / 256) for two K-steps
// m = 0, 1 of 8 bytes; the query is split f16 hi + lo as k_query_fragments_fp8 does; combine, then x 256.
__device__ inline float rescore_chain(const float* __restrict__ q, const Fp8WidenRow* __restrict__ x_row, int D, int n, int g) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4* xp = reinterpret_cast<const u32x4*>(x_row) + g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc_lo = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < D / 64; ++j) {
        const u32x4 w = xp[j * 4];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            u32x4 h;
            h[0] = fp8x2_to_f16x2_scaled(w[2 * m], 0x010C000Cu);
            h[1] = fp8x2_to_f16x2_scaled(w[2 * m], 0x030C020Cu);
            h[2] = fp8x2_to_f16x2_scaled(w[2 * m + 1], 0x010C000Cu);
            h[3] = fp8x2_to_f16x2_scaled(w[2 * m + 1], 0x030C020Cu);
            const f16x8 xb = __builtin_bit_cast(f16x8, h);
            f16x8 ah, al;
#pragma unroll
            for (int e = 0; e < 8; ++e) {  // the split of k_query_fragments_fp8
                const float v = n == 0 ? q[64 * j + 16 * g + 8 * m + e] : 0.f;
                const _Float16 hv = (_Float16)v;
                ah[e] = hv;
                al[e] = (_Float16)((v - (float)hv) * kLoScale);
            }
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, xb, acc, 0, 0, 0);
            acc_lo = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, xb, acc_lo, 0, 0, 0);
        }
    }
    return fmaf(acc_lo[0], 1.0f / kLoScale, acc[0]) * 256.0f;
}

// kIdxFp8Mfma: the row's bytes as they are against the query's two e4m3 pieces (fp8n_*: what k_query_fragments_fp8n
// writes), one accumulator per piece, combined as the scan's epilogue combines them.
__device__ inline float rescore_chain(const float* __restrict__ q, const Fp8MfmaRow* __restrict__ x_row, int D, int n, int g) {
    const int lane = g * 16 + n;
    float s1, s2;
    fp8n_query_scales(q, D, true, lane, 64, [](float v) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
        return v;
    }, s1, s2);
    const uint64_t* xp = reinterpret_cast<const uint64_t*>(x_row) + 2 * g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc_lo = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < D / 64; ++j) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const long xb = (long)xp[j * 8 + m];
            uint64_t w1 = 0, w2 = 0;
            if (n == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = q[64 * j + 16 * g + 8 * m + e];
                    const uint32_t b1 = fp8n_piece1(v, s1);
                    w1 |= (uint64_t)b1 << (8 * e);
                    w2 |= (uint64_t)fp8n_piece2(v, s1, b1, s2) << (8 * e);
                }
            }
            acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8((long)w1, xb, acc, 0, 0, 0);
            acc_lo = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8((long)w2, xb, acc_lo, 0, 0, 0);
        }
    }
    return fmaf(acc_lo[0], s2, acc[0] * s1);
}

// exact[qi][c] = chain(q[qi], idx[ids[qi * id_stride + c]]) * row_scale for c < kk, -inf where the list has no entry:
// beyond cand_cnt[qi] when a count is given (the GEMM path's int32 lists), else where the id is negative (the
// two-stage path's int64 lists, padded with -1).
template <class RowT, class IdT>
__global__ __launch_bounds__(256) void k_rescore(const float* __restrict__ q, int D, const RowT* __restrict__ idx,
                                                 const float* __restrict__ row_scale, const IdT* __restrict__ ids, int id_stride,
                                                 const int32_t* __restrict__ cand_cnt, int Q, int kk,
                                                 float* __restrict__ exact /* [Q, kk] */) {
    const int lane = threadIdx.x & 63;
    const int n = lane & 15, g = lane >> 4;
    const int tiles = (kk + 15) / 16;
    const int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= (int64_t)Q * tiles) return;  // whole waves only: the MFMAs below run with all 64 lanes
    const int qi = (int)(w / tiles), t = (int)(w % tiles);
    const int m = cand_cnt && cand_cnt[qi * kCntStride] < kk ? cand_cnt[qi * kCntStride] : kk;
    const int c = t * 16 + n;
    const IdT row = c < m ? ids[(int64_t)qi * id_stride + c] : -1;
    const float dot = rescore_chain(q + (int64_t)qi * D, idx + (int64_t)(row >= 0 ? row : 0) * D, D, n, g);
    if (g == 0 && c < kk) {
        float s = -INFINITY;
        if (row >= 0) s = row_scale ? dot * row_scale[row] : dot;
        exact[(int64_t)qi * kk + c] = s;
    }
}

template <class RowT, class IdT>
static void launch_rescore(int timing_class, hipStream_t st, const float* q, int D, const void* idx, const float* row_scale,
                           const IdT* ids, int id_stride, const int32_t* cand_cnt, int Q, int kk, float* exact) {
    const int tiles = (kk + 15) / 16;
    const int64_t waves = (int64_t)Q * tiles;
    launch_timed(timing_class, k_rescore<RowT, IdT>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, q, D,
                 static_cast<const RowT*>(idx), row_scale, ids, id_stride, cand_cnt, Q, kk, exact);
}

// final selection on the exact scores: (score desc, row id asc), like the scan
__global__ __launch_bounds__(kSelectThreads) void k_gt_final(const float* __restrict__ exact, const int32_t* __restrict__ cand_id,
                                                             const int32_t* __restrict__ cand_cnt, int kk, int k,
                                                             int64_t row_id_base, float* __restrict__ out_score,
                                                             int64_t* __restrict__ out_index) {
    __shared__ SelectShared sh;
    const int qi = blockIdx.x;
    const int m0 = cand_cnt[qi * kCntStride] < kk ? cand_cnt[qi * kCntStride] : kk;
    const float* es = exact + (int64_t)qi * kk;
    const int32_t* ci = cand_id + (int64_t)qi * kGemmTopkCap;
    auto load = [&](int64_t i) -> uint64_t { return make_key(es[i], (uint32_t)ci[i]); };
    const int m = block_topk(sh, load, m0, k);
    write_topk(sh, m, qi, k, row_id_base, out_score, out_index);
}

struct GtLayout {
    size_t tau, cnt, cs, ci, exact, scores, wsplit, total;
    int64_t slab;
};

static GtLayout gt_layout(int Q, int64_t N, int D, int k, int single = 1 /* the larger reserve */) {
    GtLayout L;
    Bump m;
    const int kk = gemm_topk_reserve(k, single) <= EVI_TOPK_MAX_K ? gemm_topk_reserve(k, single) : gemm_topk_reserve(k, 0);
    L.slab = N < kGemmSlabRows ? (N > 0 ? N : 1) : kGemmSlabRows;
    const int64_t first = N < kGemmFirstRows ? (N > 0 ? N : 1) : kGemmFirstRows;
    L.tau = m.take((size_t)Q * sizeof(float));
    L.cnt = m.take((size_t)Q * kCntStride * sizeof(int32_t));
    L.cs = m.take((size_t)Q * kGemmTopkCap * sizeof(float));
    L.ci = m.take((size_t)Q * kGemmTopkCap * sizeof(int32_t));
    L.exact = m.take((size_t)Q * kk * sizeof(float));
    L.scores = m.take((size_t)first * Q * sizeof(float));  // only the first slab's scores are materialised
    L.wsplit = m.take(gemm_bf16x3_workspace_bytes(Q, D));
    L.total = m.total;
    return L;
}

}  // namespace evi

extern "C" size_t evi_cosine_topk_gemm_workspace_bytes(int Q, int64_t N, int D, int k) {
    if (Q <= 0 || N < 0 || D <= 0 || k <= 0) return 0;
    return gt_layout(Q, N, D, k).total;
}

__global__ void k_shadow_bf16(const float* __restrict__ x, int64_t n, __bf16* __restrict__ out) {
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (int64_t)gridDim.x * blockDim.x * 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + i);
        typedef __bf16 bf16x4v __attribute__((ext_vector_type(4)));
        bf16x4v o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (__bf16)v[e];
        *reinterpret_cast<bf16x4v*>(out + i) = o;
    }
}

extern "C" int evi_index_shadow_bf16(const float* idx, int64_t N, int D, void* out_bf16, void* stream) {
    EVI_REQUIRE(N >= 0 && D >= 1, "evi_index_shadow_bf16: need N >= 0 and D >= 1");
    if (D % 4 != 0) return fail(EVI_ERR_UNSUPPORTED, "evi_index_shadow_bf16: D must be a multiple of 4, got %d", D);
    if (N == 0) return EVI_OK;
    EVI_REQUIRE(idx && out_bf16, "evi_index_shadow_bf16: null pointer");
    hipLaunchKernelGGL(k_shadow_bf16, dim3(4096), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), idx, N * D,
                       static_cast<__bf16*>(out_bf16));
    EVI_LAUNCH_CHECK();
    return EVI_OK;
}

// Query planes of the many-query selection over an e4m3 index in its NATIVE scan variant: hi = s1 p1, lo = s2 p2, the two
// dequantised pieces the scan multiplies (fp8n_*).  An e4m3 value times a power of two is exactly a bf16 value, so the
// selection's ideal score equals the scan's and the two differ by accumulation order only.  One workgroup per query.
__global__ __launch_bounds__(256) void k_fp8n_query_planes(const float* __restrict__ q, int D, int Kp, __bf16* __restrict__ hi,
                                                           __bf16* __restrict__ lo) {
    __shared__ float red[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float* qr = q + (int64_t)i * D;
    float s1, s2;
    fp8n_query_scales(qr, D, true, tid, 256, [&](float v) { return block256_max(red, tid, v); }, s1, s2);
    for (int d = tid; d < Kp; d += 256) {
        float p1 = 0.f, p2 = 0.f;
        if (d < D) {
            const uint32_t b1 = fp8n_piece1(qr[d], s1);
            p1 = s1 * e4m3_to_float(b1);
            p2 = s2 * e4m3_to_float(fp8n_piece2(qr[d], s1, b1, s2));
        }
        hi[(int64_t)i * Kp + d] = (__bf16)p1;
        lo[(int64_t)i * Kp + d] = (__bf16)p2;
    }
}

// the query planes the selection GEMM multiplies, in `wsplit`: the bf16 hi / lo split of the f32 query, or (native e4m3
// variant) the scan's own two pieces
static int gt_query_planes(IndexKind kind, const float* q, int Q, int D, void* wsplit, hipStream_t st) {
    if (kind != kIdxFp8Mfma) return split_weight_bf16x3(q, Q, D, D, wsplit, st);  // the queries are the "weights": split once
    __bf16 *hi, *lo;
    int Kp;
    bf16x3_planes(wsplit, Q, D, &hi, &lo, &Kp);
    hipLaunchKernelGGL(k_fp8n_query_planes, dim3(Q), dim3(256), 0, st, q, D, Kp, hi, lo);
    EVI_LAUNCH_CHECK();
    return EVI_OK;
}

// scores [rows, Q] *= row_scale[row], as k_gt_filter scales them
__global__ void k_gt_scale_rows(float* __restrict__ scores, int64_t rows, int Q, const float* __restrict__ row_scale) {
    const int64_t total = rows * Q;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        scores[i] *= row_scale[i / Q];
}

// row_labels / query_allow (both or neither): the row filter of the scan.  A hidden (query, row) pair is never appended
// to a list, so the lists, the thresholds, the gap test and the rescore speak of the rows visible to each query only — the
// compacted index.  A query with fewer than kk visible rows keeps tau = -inf to the end (tau is raised only on a list of kk
// real entries), every slab appends all of its visible rows, and the final writer pads with (-inf, -1).
static int cosine_topk_gemm_impl(const float* q, int Q, const void* idx, IndexKind kind, int products, const void* shadow, int64_t N,
                                 int D, const float* row_scale, int k, int64_t row_id_base, float* out_score,
                                 int64_t* out_index, int32_t* status, void* workspace, size_t workspace_bytes, void* stream,
                                 const uint8_t* row_labels = nullptr, const uint32_t* query_allow = nullptr) {
    EVI_REQUIRE((row_labels == nullptr) == (query_allow == nullptr), "evi_cosine_topk_gemm: row_labels and query_allow go together");
    EVI_REQUIRE(products == 1 || products == 3, "evi_cosine_topk_gemm: products must be 3 (split-bf16) or 1 (plain bf16), got %d",
                products);
    const int single = products == 1;
    const int f16 = kind == kIdxF16;
    const bool fp8 = kind >= kIdxFp8Widen;  // e4m3 rows: one selection precision (products = 3 runs two, see gemm_bf16x3.hip)
    EVI_REQUIRE(!shadow || (single && kind == kIdxF32), "evi_cosine_topk_gemm: a bf16 shadow goes with an f32 index and products = 1");
    EVI_REQUIRE(!fp8 || (!single && row_scale), "evi_cosine_topk_gemm_fp8: row_scale (the per-row dequantisation scale) is required");
    EVI_REQUIRE(Q >= 1 && N >= 1 && D >= 1, "evi_cosine_topk_gemm: need Q >= 1, N >= 1, D >= 1, got Q=%d N=%lld D=%d", Q,
                (long long)N, D);
    EVI_REQUIRE(k >= 1, "evi_cosine_topk_gemm: k must be >= 1, got %d", k);
    if (fp8 && (D % 64 != 0 || D > 1280))
        return fail(EVI_ERR_UNSUPPORTED, "evi_cosine_topk_gemm_fp8: D must be a multiple of 64 up to 1280, got %d", D);
    if (D % (f16 ? 32 : 16) != 0)
        return fail(EVI_ERR_UNSUPPORTED, "evi_cosine_topk_gemm: D must be a multiple of %d, got %d", f16 ? 32 : 16, D);
    const int kk = gemm_topk_reserve(k, single);
    if (kk > EVI_TOPK_MAX_K)
        return fail(EVI_ERR_UNSUPPORTED, "evi_cosine_topk_gemm: k + reserve = %d exceeds %d (k <= %d with products = %d)", kk,
                    EVI_TOPK_MAX_K, single ? EVI_TOPK_MAX_K - 1024 : EVI_TOPK_MAX_K * 2 / 3, products);
    EVI_REQUIRE(N < (int64_t)0x7FFFFFFF, "evi_cosine_topk_gemm: N must fit int32 row ids");
    EVI_REQUIRE(q && idx && out_score && out_index && status && workspace, "evi_cosine_topk_gemm: null pointer");
    const GtLayout L = gt_layout(Q, N, D, k);
    if (workspace_bytes < L.total)
        return fail(EVI_ERR_NOMEM, "evi_cosine_topk_gemm: workspace %zu B < %zu B", workspace_bytes, L.total);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(workspace);
    float* tau = reinterpret_cast<float*>(base + L.tau);
    int32_t* cnt = reinterpret_cast<int32_t*>(base + L.cnt);
    float* cs = reinterpret_cast<float*>(base + L.cs);
    int32_t* ci = reinterpret_cast<int32_t*>(base + L.ci);
    float* exact = reinterpret_cast<float*>(base + L.exact);
    float* scores = reinterpret_cast<float*>(base + L.scores);
    // selection operand: the index itself, or its bf16 shadow (same arithmetic as products = 1, no conversion work)
    const int a_kind = fp8 ? 3 : (shadow ? 2 : f16);
    const char* rows_base = static_cast<const char*>(shadow ? shadow : idx);
    const size_t row_bytes = (size_t)D * (fp8 ? 1 : (a_kind ? 2 : 4));
    hipLaunchKernelGGL(k_gt_init, dim3((Q + 255) / 256), dim3(256), 0, st, tau, cnt, Q, status);
    EVI_LAUNCH_CHECK();
    int rc = gt_query_planes(kind, q, Q, D, base + L.wsplit, st);
    if (rc != EVI_OK) return rc;
    // Slab growth.  Unfiltered, a slab of g times the rows seen so far appends about g kk rows to a list of kk.  A filter of
    // independent labels thins the slab and the rows behind tau alike, so the expectation stands; while a query has seen
    // fewer than kk visible rows its tau is still -inf and it takes every visible row of the slab, which is fewer than g kk.
    // Either way the list needs (1 + g) kk slots: the filtered call lowers g until that is inside 8/9 of the capacity (kk up
    // to 1618 keeps 8; kk = 2048 gets 6), since its overflow costs a whole filtered scan.
    int growth = kGemmGrowth;
    if (row_labels)
        while (growth > 2 && (int64_t)kk * (1 + growth) * 9 > (int64_t)kGemmTopkCap * 8) --growth;
    int64_t begin = 0, seg = N < kGemmFirstRows ? N : kGemmFirstRows;
    while (begin < N) {
        const int64_t rows = (N - begin) < seg ? (N - begin) : seg;
        const void* slab = rows_base + begin * row_bytes;
        if (begin == 0) {
            // first slab: every score passes (tau = -inf), so form the scores and append them with plain stores
            rc = launch_gemm_bf16_presplit(slab, a_kind, single, rows, D, D, base + L.wsplit, Q, scores, Q, st);
            if (rc != EVI_OK) return rc;
            int64_t blocks = (rows * Q + 255) / 256;
            if (blocks > 8192) blocks = 8192;
            if (row_labels)
                hipLaunchKernelGGL(k_gt_filter<true>, dim3((unsigned)blocks), dim3(256), 0, st, scores, rows, Q, begin, row_scale,
                                   tau, cs, ci, cnt, status, row_labels, query_allow);
            else
                hipLaunchKernelGGL(k_gt_filter<false>, dim3((unsigned)blocks), dim3(256), 0, st, scores, rows, Q, begin, row_scale,
                                   tau, cs, ci, cnt, status, (const uint8_t*)nullptr, (const uint32_t*)nullptr);
        } else {
            // later slabs: scores ~ idx[begin + r] . q[i] never leave the registers of the GEMM — its epilogue
            // compares them with tau and appends the few survivors
            const GemmFilter flt{tau, row_scale, begin, cs, ci, cnt, status, kGemmTopkCap, kCntStride, row_labels, query_allow};
            rc = launch_gemm_bf16x3_filter(slab, a_kind, single, rows, D, D, base + L.wsplit, Q, flt, st);
            if (rc != EVI_OK) return rc;
        }
        hipLaunchKernelGGL(k_gt_clamp, dim3((Q + 255) / 256), dim3(256), 0, st, cnt, Q);
        hipLaunchKernelGGL(k_candidates_select, dim3(Q), dim3(kSelectThreads), 0, st, cs, ci, cnt, tau,
                           (int64_t)kGemmTopkCap, kk, (int64_t)-1, 0, row_id_base, (float*)nullptr, (int64_t*)nullptr,
                           (const int32_t*)nullptr);
        EVI_LAUNCH_CHECK();
        begin += rows;
        int64_t next = begin * growth;
        seg = next < L.slab ? next : L.slab;
    }
    hipLaunchKernelGGL(k_gt_gap, dim3(Q), dim3(64), 0, st, q, Q, D, cs, cnt, k, kk,
                       fp8 ? kApproxEpsFp8 : (single ? kApproxEps1 : kApproxEps), kind == kIdxFp8Widen ? 1 : 0, status);
    if (kind == kIdxFp8Mfma)
        launch_rescore<Fp8MfmaRow>(kUntimed, st, q, D, idx, row_scale, ci, kGemmTopkCap, cnt, Q, kk, exact);
    else if (kind == kIdxFp8Widen)
        launch_rescore<Fp8WidenRow>(kUntimed, st, q, D, idx, row_scale, ci, kGemmTopkCap, cnt, Q, kk, exact);
    else if (f16)
        launch_rescore<_Float16>(kUntimed, st, q, D, idx, row_scale, ci, kGemmTopkCap, cnt, Q, kk, exact);
    else
        launch_rescore<float>(kUntimed, st, q, D, idx, row_scale, ci, kGemmTopkCap, cnt, Q, kk, exact);
    hipLaunchKernelGGL(k_gt_final, dim3(Q), dim3(kSelectThreads), 0, st, exact, ci, cnt, kk, k, row_id_base, out_score,
                       out_index);
    EVI_LAUNCH_CHECK();
    return EVI_OK;
}

extern "C" int evi_cosine_topk_gemm(const float* q, int Q, const float* idx, int64_t N, int D, const float* row_scale,
                                    int k, int64_t row_id_base, int products, const void* shadow_bf16, float* out_score,
                                    int64_t* out_index, int32_t* status, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    return cosine_topk_gemm_impl(q, Q, idx, kIdxF32, products, shadow_bf16, N, D, row_scale, k, row_id_base, out_score, out_index,
                                 status, workspace, workspace_bytes, stream);
}

extern "C" int evi_cosine_topk_gemm_f16(const float* q, int Q, const void* idx_f16, int64_t N, int D, const float* row_scale,
                                        int k, int64_t row_id_base, int products, float* out_score, int64_t* out_index,
                                        int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    return cosine_topk_gemm_impl(q, Q, idx_f16, kIdxF16, products, nullptr, N, D, row_scale, k, row_id_base, out_score, out_index,
                                 status, workspace, workspace_bytes, stream);
}

extern "C" int evi_cosine_topk_gemm_fp8(const float* q, int Q, const void* idx_fp8, int64_t N, int D, const float* row_scale,
                                        int k, int64_t row_id_base, int native_mfma, float* out_score, int64_t* out_index,
                                        int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    return cosine_topk_gemm_impl(q, Q, idx_fp8, native_mfma ? kIdxFp8Mfma : kIdxFp8Widen, 3, nullptr, N, D, row_scale, k,
                                 row_id_base, out_score, out_index, status, workspace, workspace_bytes, stream);
}

extern "C" int evi_cosine_topk_gemm_filtered(const float* q, int Q, const void* idx, int kind, int64_t N, int D,
                                             const float* row_scale, const uint8_t* row_labels, const uint32_t* query_allow,
                                             int k, int64_t row_id_base, int products, const void* shadow_bf16, float* out_score,
                                             int64_t* out_index, int32_t* status, void* workspace, size_t workspace_bytes,
                                             void* stream) {
    EVI_REQUIRE(kind >= 0 && kind <= 3, "evi_cosine_topk_gemm_filtered: kind must be 0 (f32), 1 (f16), 2 (e4m3 widened) or 3 (e4m3 "
                "native), got %d", kind);
    EVI_REQUIRE(row_labels && query_allow, "evi_cosine_topk_gemm_filtered: null row_labels / query_allow");
    EVI_REQUIRE(kind < 2 || (products == 3 && !shadow_bf16),
                "evi_cosine_topk_gemm_filtered: an e4m3 index has one selection precision (products = 3) and no bf16 shadow");
    static const IndexKind kinds[4] = {kIdxF32, kIdxF16, kIdxFp8Widen, kIdxFp8Mfma};
    return cosine_topk_gemm_impl(q, Q, idx, kinds[kind], products, shadow_bf16, N, D, row_scale, k, row_id_base, out_score,
                                 out_index, status, workspace, workspace_bytes, stream, row_labels, query_allow);
}

extern "C" int evi_cosine_topk_gemm_fp8_selection(const float* q, int Q, const void* idx_fp8, int64_t N, int D,
                                                  const float* row_scale, int native_mfma, float* out_scores, void* workspace,
                                                  size_t workspace_bytes, void* stream) {
    EVI_REQUIRE(Q >= 1 && N >= 1, "evi_cosine_topk_gemm_fp8_selection: need Q >= 1 and N >= 1, got Q=%d N=%lld", Q, (long long)N);
    if (D < 64 || D % 64 != 0 || D > 1280)
        return fail(EVI_ERR_UNSUPPORTED, "evi_cosine_topk_gemm_fp8_selection: D must be a multiple of 64 up to 1280, got %d", D);
    EVI_REQUIRE(q && idx_fp8 && row_scale && out_scores && workspace, "evi_cosine_topk_gemm_fp8_selection: null pointer");
    if (workspace_bytes < gemm_bf16x3_workspace_bytes(Q, D))
        return fail(EVI_ERR_NOMEM, "evi_cosine_topk_gemm_fp8_selection: workspace %zu B < %zu B", workspace_bytes,
                    gemm_bf16x3_workspace_bytes(Q, D));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int rc = gt_query_planes(native_mfma ? kIdxFp8Mfma : kIdxFp8Widen, q, Q, D, workspace, st);
    if (rc != EVI_OK) return rc;
    rc = launch_gemm_bf16_presplit(idx_fp8, 3, 0, N, D, D, workspace, Q, out_scores, Q, st);
    if (rc != EVI_OK) return rc;
    int64_t blocks = (N * Q + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_gt_scale_rows, dim3((unsigned)blocks), dim3(256), 0, st, out_scores, N, Q, row_scale);
    EVI_LAUNCH_CHECK();
    return EVI_OK;
}

// =====================================================================================================
// Two-stage exact scan (f16 shadow selection + f32 re-scoring): the result of evi_cosine_topk at half
// the HBM bytes per batch.
//
// The f32 index is kept as it is and an f16 copy of it (the shadow, rn(x) element by element, made once
// by evi_index_shadow_f16: + 50 % memory) is what the scan streams.  Stage 1 is evi_cosine_topk_f16
// over the shadow with kk = k + reserve results per query.  For rows of norm <= 1 its scores differ
// from the f32 scan's by at most kShadowEps * |q|:
//     |q . (x - rn_f16(x))| <= 2^-11 |q| |x|                    (Cauchy-Schwarz, f16 has 11 significant bits)
//     f32 chain of the exact scan: 768 roundings x 2^-23         (truncating adders assumed)
//     f16-MFMA chain of the shadow scan + the hi/lo query split: < 5e-5
// so when approx[k-1] - approx[kk-1] > 2 eps |q| every row outside the kk kept ones is beaten, in exact
// score, by k kept rows: the true top-k is inside the list (same argument as the many-query path above).
// Stage 2 re-scores the kk rows from the f32 index with the scan's own v_mfma_f32_16x16x4_f32 chain and
// takes the top-k on those scores: ids and scores bit-identical to evi_cosine_topk.  A failed proof
// ORs 1 into *status (sticky: the caller zeroes it, so a pipeline of batches can share one flag and read it
// once) and the caller runs the f32 scan.
// =====================================================================================================
namespace evi {

constexpr float kShadowEps = 7.0e-4f;

static int two_stage_kk(int k) { return gemm_topk_reserve(k, 0); }

__global__ void k_shadow_f16(const float* __restrict__ x, int64_t n, _Float16* __restrict__ out) {
    // 4 elements per thread per step: one 16-byte load, one 8-byte store
    const int64_t n4 = n >> 2;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    f16x4* o4 = reinterpret_cast<f16x4*>(out);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const f32x4 v = x4[i];
        f16x4 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) h[e] = (_Float16)v[e];  // round to nearest even
        o4[i] = h;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (_Float16)x[i];
}

// Final top-k on the exact scores, and the proof: approx / ids are the [Q, kk] lists evi_cosine_topk_f16 wrote (sorted,
// (-inf, -1) past the end of a short index); the true top-k is among them when approx[k-1] - approx[kk-1] > 2 eps |q|.
__global__ __launch_bounds__(kSelectThreads) void k_ts_final(const float* __restrict__ exact, const int64_t* __restrict__ ids,
                                                             int kk, int k, int64_t row_id_base, float* __restrict__ out_score,
                                                             int64_t* __restrict__ out_index, const float* __restrict__ q, int D,
                                                             const float* __restrict__ approx, float eps,
                                                             int32_t* __restrict__ status, int32_t* __restrict__ call_flag) {
    __shared__ SelectShared sh;
    const int qi = blockIdx.x;
    const float* es = exact + (int64_t)qi * kk;
    const int64_t* ci = ids + (int64_t)qi * kk;
    if (threadIdx.x < 64) {  // wave 0: the gap test
        const int lane = threadIdx.x;
        const float ss = wave_sumsq(q + (int64_t)qi * D, D, lane);
        if (lane == 0 && ci[kk - 1] >= 0) {  // otherwise every row of the index is in the list
            const float* s = approx + (int64_t)qi * kk;
            // the bound is relative to |q| and assumes the f16 hi / lo split of the query keeps its 22 bits: far from unit
            // norm (elements near the f16 subnormal range, or the 2048 x lo part near overflow) it does not hold, and the
            // proof is refused — the f32 scan then does the batch
            const bool norm_ok = ss >= 0.0625f && ss <= 16.0f;
            if (gap_fails(s[k - 1] - s[kk - 1], eps, ss) || !norm_ok) {  // also catches NaN scores
                if (status) atomicOr(status, 1);  // the caller's sticky flag (a pipeline of batches shares it)
                atomicOr(call_flag, 1);           // this call's own flag: opens the gate of the fallback scan
            }
        }
    }
    auto load = [&](int64_t i) -> uint64_t { return ci[i] >= 0 ? make_key(es[i], (uint32_t)ci[i]) : 0ull; };
    const int m = block_topk(sh, load, kk, k);
    write_topk(sh, m, qi, k, row_id_base, out_score, out_index);
}

struct TsLayout {
    size_t flag, approx, ids, exact, scan, scan_bytes, total;
};
static TsLayout ts_layout(int Q, int64_t N, int D, int k) {
    TsLayout L;
    const int kk = two_stage_kk(k);
    Bump m;
    L.flag = m.take(sizeof(int32_t));  // this call's proof flag (gate of the device-side fallback)
    L.approx = m.take((size_t)Q * kk * sizeof(float));
    L.ids = m.take((size_t)Q * kk * sizeof(int64_t));
    L.exact = m.take((size_t)Q * kk * sizeof(float));
    L.scan_bytes = evi_cosine_topk_workspace_bytes(Q, N, D, kk);
    L.scan = m.take(L.scan_bytes);
    L.total = m.total;
    return L;
}

}  // namespace evi

extern "C" int evi_index_shadow_f16(const float* idx, int64_t N, int D, void* out_f16, void* stream) {
    EVI_REQUIRE(N >= 0 && D >= 1, "evi_index_shadow_f16: need N >= 0, D >= 1");
    if (N == 0) return EVI_OK;
    EVI_REQUIRE(idx && out_f16, "evi_index_shadow_f16: null pointer");
    hipLaunchKernelGGL(k_shadow_f16, dim3(4096), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), idx, N * D,
                       static_cast<_Float16*>(out_f16));
    EVI_LAUNCH_CHECK();
    return EVI_OK;
}

extern "C" size_t evi_cosine_topk_two_stage_workspace_bytes(int Q, int64_t N, int D, int k) {
    if (Q <= 0 || N < 0 || D <= 0 || k <= 0 || two_stage_kk(k) > EVI_TOPK_MAX_K) return 0;
    return ts_layout(Q, N, D, k).total;
}

static int cosine_topk_two_stage_impl(const float* q, int Q, const float* idx, const void* shadow_f16, int64_t N, int D,
                                      const uint8_t* row_labels, const uint32_t* query_allow, int k, int64_t row_id_base,
                                      float* out_score, int64_t* out_index, int32_t* status, int device_fallback, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    EVI_REQUIRE(Q >= 1 && N >= 1, "evi_cosine_topk_two_stage: need Q >= 1 and N >= 1, got Q=%d N=%lld", Q, (long long)N);
    EVI_REQUIRE(k >= 1, "evi_cosine_topk_two_stage: k must be >= 1, got %d", k);
    if (D < 32 || D % 32 != 0 || D > 1280)
        return fail(EVI_ERR_UNSUPPORTED, "evi_cosine_topk_two_stage: D must be a multiple of 32 in [32, 1280], got %d", D);
    const int kk = two_stage_kk(k);
    if (kk > EVI_TOPK_MAX_K)
        return fail(EVI_ERR_UNSUPPORTED, "evi_cosine_topk_two_stage: k + reserve = %d exceeds %d (k <= %d)", kk, EVI_TOPK_MAX_K,
                    EVI_TOPK_MAX_K * 2 / 3);
    EVI_REQUIRE(q && idx && shadow_f16 && out_score && out_index && workspace, "evi_cosine_topk_two_stage: null pointer");
    EVI_REQUIRE(status || device_fallback,
                "evi_cosine_topk_two_stage: without the device-side fallback the caller must pass a status word and check it");
    const TsLayout L = ts_layout(Q, N, D, k);
    if (workspace_bytes < L.total)
        return fail(EVI_ERR_NOMEM, "evi_cosine_topk_two_stage: workspace %zu B < %zu B", workspace_bytes, L.total);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(workspace);
    float* approx = reinterpret_cast<float*>(base + L.approx);
    int64_t* ids = reinterpret_cast<int64_t*>(base + L.ids);
    float* exact = reinterpret_cast<float*>(base + L.exact);
    int32_t* call_flag = reinterpret_cast<int32_t*>(base + L.flag);
    EVI_HIP_CHECK(hipMemsetAsync(call_flag, 0, sizeof(int32_t), st));
    // stage 1: kk best rows per query by shadow score (local row ids)
    const int rc = cosine_topk_impl(q, Q, shadow_f16, kIdxF16, N, D, nullptr, kk, 0, approx, ids, base + L.scan, L.scan_bytes, stream,
                                    nullptr, row_labels, query_allow);
    if (rc != EVI_OK) return rc;
    // stage 2: exact scores from the f32 rows, final top-k + proof
    launch_rescore<float>(kTimeSelect, st, q, D, idx, nullptr, ids, kk, nullptr, Q, kk, exact);
    launch_timed(kTimeSelect, k_ts_final, dim3(Q), dim3(kSelectThreads), 0, st, exact, ids, kk, k, row_id_base, out_score,
                 out_index, q, D, approx, kShadowEps, status, call_flag);
    EVI_LAUNCH_CHECK();
    if (device_fallback) {
        // The f32 scan of the same batch into the same outputs, gated on this call's flag: while the proof held every
        // kernel returns at once (a few empty launches); when it failed the scan overwrites the unproven result before any
        // later work of the stream can read it.  No read-back, no agreement between ranks needed: each shard's record is
        // exact when it leaves the device.  The stage-1 scan workspace is free again and large enough (kk >= k).
        const int rc2 = cosine_topk_impl(q, Q, idx, kIdxF32, N, D, nullptr, k, row_id_base, out_score, out_index, base + L.scan,
                                         L.scan_bytes, stream, call_flag, row_labels, query_allow);
        if (rc2 != EVI_OK) return rc2;
    }
    return EVI_OK;
}

extern "C" int evi_cosine_topk_two_stage(const float* q, int Q, const float* idx, const void* shadow_f16, int64_t N, int D,
                                         int k, int64_t row_id_base, float* out_score, int64_t* out_index, int32_t* status,
                                         int device_fallback, void* workspace, size_t workspace_bytes, void* stream) {
    return cosine_topk_two_stage_impl(q, Q, idx, shadow_f16, N, D, nullptr, nullptr, k, row_id_base, out_score, out_index, status,
                                      device_fallback, workspace, workspace_bytes, stream);
}

// The filter goes to the stage-1 shadow scan (the kk kept rows are the best VISIBLE rows by shadow score, so the proof is
// the unfiltered one over the visible rows) and to the gated f32 fallback scan; the re-scoring, the gap test and the final
// selection see a shorter or -1 padded list exactly as they do for a short index.
extern "C" int evi_cosine_topk_two_stage_filtered(const float* q, int Q, const float* idx, const void* shadow_f16, int64_t N,
                                                  int D, const uint8_t* row_labels, const uint32_t* query_allow, int k,
                                                  int64_t row_id_base, float* out_score, int64_t* out_index, int32_t* status,
                                                  int device_fallback, void* workspace, size_t workspace_bytes, void* stream) {
    EVI_REQUIRE(row_labels && query_allow, "evi_cosine_topk_two_stage_filtered: null row_labels / query_allow");
    return cosine_topk_two_stage_impl(q, Q, idx, shadow_f16, N, D, row_labels, query_allow, k, row_id_base, out_score, out_index,
                                      status, device_fallback, workspace, workspace_bytes, stream);
}

// =====================================================================================================
// Per-query candidate lists: the exact top-k of the rows a query NAMES (a packed batch's node_embedding_ids cut by ptr,
// edge_attr cut by edge_ptr) instead of the rows of the whole index — the reference's per-group arg-max
// (scripts/build_retrieval_pipeline.py:856-874), generalised as evi_cosine_topk generalised it.
//
//   k_cand_ptr / k_cand_mark   cand_ptr checked, ids -> local rows + drop mask (the id rules of the header)
//   evi_first_occurrence + evi_first_seen_rank (compact.hip)   per query: the distinct rows and their count
//   k_cand_tiles               exclusive prefix of ceil(count / 16): which wave of the scoring grid serves which query
//   k_cand_score               the ragged k_rescore: one wave per 16 distinct rows, the same chains -> the scan's bits
//   k_cand_select              block_topk over a query's compacted (score, local row) pairs, write_topk
//
// Every grid comes from Q, T and k; nothing is read back.  Bound: the gather of the distinct rows (whole rows at random
// places of HBM), then launch latency — seven short launches per call.
// =====================================================================================================
namespace evi {

constexpr int kCandThreads = 1024;

// seg_ptr = cand_ptr when 0 <= cand_ptr[i] <= cand_ptr[i + 1] <= T for every i; else every list is EMPTY and bit 2 goes
// into *status.  (Clamping list by list would keep every read inside cand_ids, but lists that overlap would share their
// de-duplication tables: a malformed call answers nothing instead of something that depends on the interleaving.)
__global__ __launch_bounds__(kCandThreads) void k_cand_ptr(const int64_t* __restrict__ cand_ptr, int Q, int64_t T,
                                                           int64_t* __restrict__ seg_ptr, int32_t* __restrict__ status) {
    int bad = 0;
    for (int i = threadIdx.x; i < Q; i += kCandThreads) {
        const int64_t a = cand_ptr[i], b = cand_ptr[i + 1];
        bad |= (a < 0 || b < a || b > T) ? 1 : 0;
    }
    const int any = __syncthreads_or(bad);
    for (int i = threadIdx.x; i <= Q; i += kCandThreads) seg_ptr[i] = any ? 0 : cand_ptr[i];
    if (any && threadIdx.x == 0 && status) atomicOr(status, 2);
}

// The id rules, before any address is formed from an id: g < 0 padding; g >= id_limit dropped + status bit 1;
// g - row_id_base outside [0, N) not on this shard; else local row g - row_id_base.
__global__ __launch_bounds__(256) void k_cand_mark(const int64_t* __restrict__ cand_ids, int64_t T, int64_t N, int64_t row_id_base,
                                                   int64_t id_limit, int64_t* __restrict__ keys, uint8_t* __restrict__ drop,
                                                   int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T) return;
    const int64_t g = cand_ids[i];
    const bool over = g >= 0 && g >= id_limit;
    // g >= row_id_base: the difference is in [0, 2^64), exact in unsigned arithmetic whatever the signs
    const uint64_t local = (uint64_t)g - (uint64_t)row_id_base;
    const bool keep = g >= 0 && !over && g >= row_id_base && local < (uint64_t)N;
    keys[i] = keep ? (int64_t)local : 0;
    drop[i] = keep ? 0 : 1;
    if (over && status) atomicOr(status, 1);
}

// tile_pre[i] = sum_{j < i} ceil(count[j] / 16), i = 0 .. Q: one workgroup, chunks of 1024 queries.
__global__ __launch_bounds__(kCandThreads) void k_cand_tiles(const int32_t* __restrict__ count, int Q, int32_t* __restrict__ tile_pre) {
    __shared__ int wave_tot[kCandThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int c0 = 0; c0 < Q; c0 += kCandThreads) {
        const int i = c0 + tid;
        const int v = i < Q ? (count[i] + 15) / 16 : 0;
        int incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        __syncthreads();  // wave_tot may still be read from the previous chunk
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kCandThreads / 64; ++w) {
            const int c = wave_tot[w];
            if (w < wave) before += c;
            tot += c;
        }
        if (i < Q) tile_pre[i] = base + before + incl - v;
        base += tot;
    }
    if (tid == 0) tile_pre[Q] = base;
}

// scores[p0 + c] = chain(q[qi], idx[row]) * row_scale[row], rows[p0 + c] = row for the c-th distinct row of query qi
// (p0 = seg_ptr[qi], c < count[qi]).  Wave w serves tile w - tile_pre[qi] of the query whose tile range holds w; the grid
// is sized from the host bound ceil(T / 16) + Q >= tile_pre[Q] and the waves beyond leave whole.  The query sits in row 0
// of A and the 16 rows in the columns of B exactly as in k_rescore; lanes past the count read row 0 and write nothing.
template <class RowT>
__global__ __launch_bounds__(256) void k_cand_score(const float* __restrict__ q, int D, const RowT* __restrict__ idx,
                                                    const float* __restrict__ row_scale, const int64_t* __restrict__ keys,
                                                    const int64_t* __restrict__ seg_ptr, const int32_t* __restrict__ uniq_pos,
                                                    const int32_t* __restrict__ count, const int32_t* __restrict__ tile_pre, int Q,
                                                    float* __restrict__ scores, int32_t* __restrict__ rows) {
    const int lane = threadIdx.x & 63;
    const int n = lane & 15, g = lane >> 4;
    const int64_t w = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= (int64_t)tile_pre[Q]) return;  // whole waves only: the MFMAs below run with all 64 lanes
    int lo = 0, hi = Q;  // tile_pre[lo] <= w < tile_pre[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if ((int64_t)tile_pre[mid] <= w) lo = mid; else hi = mid;
    }
    const int qi = lo;
    const int64_t p0 = seg_ptr[qi];
    const int m = count[qi];
    const int c = (int)(w - tile_pre[qi]) * 16 + n;
    const int64_t row = c < m ? keys[p0 + uniq_pos[p0 + c]] : -1;
    const float dot = rescore_chain(q + (int64_t)qi * D, idx + (row >= 0 ? row : 0) * D, D, n, g);
    if (g == 0 && c < m) {
        scores[p0 + c] = row_scale ? dot * row_scale[row] : dot;
        rows[p0 + c] = (int32_t)row;
    }
}

// count == null: every list is empty (T == 0 or N == 0), the outputs are all padding.
__global__ __launch_bounds__(kSelectThreads) void k_cand_select(const float* __restrict__ scores, const int32_t* __restrict__ rows,
                                                                const int64_t* __restrict__ seg_ptr, const int32_t* __restrict__ count,
                                                                int k, int64_t row_id_base, float* __restrict__ out_score,
                                                                int64_t* __restrict__ out_index) {
    __shared__ SelectShared sh;
    const int qi = blockIdx.x;
    const int m0 = count ? count[qi] : 0;
    const int64_t p0 = count ? seg_ptr[qi] : 0;
    const float* s = scores + p0;
    const int32_t* r = rows + p0;
    auto load = [&](int64_t i) -> uint64_t { return make_key(s[i], (uint32_t)r[i]); };
    const int m = block_topk(sh, load, m0, k);
    write_topk(sh, m, qi, k, row_id_base, out_score, out_index);
}

struct CandLayout {
    size_t seg_ptr, keys, drop, first, rank, uniq_pos, count, tile_pre, scores, rows, table, table_bytes, total;
};

static CandLayout cand_layout(int Q, int64_t T) {
    CandLayout L;
    Bump m;
    L.seg_ptr = m.take((size_t)(Q + 1) * sizeof(int64_t));
    L.keys = m.take((size_t)T * sizeof(int64_t));
    L.drop = m.take((size_t)T);
    L.first = m.take((size_t)T * sizeof(int32_t));
    L.rank = m.take((size_t)T * sizeof(int32_t));
    L.uniq_pos = m.take((size_t)T * sizeof(int32_t));
    L.count = m.take((size_t)Q * sizeof(int32_t));
    L.tile_pre = m.take((size_t)(Q + 1) * sizeof(int32_t));
    L.scores = m.take((size_t)T * sizeof(float));
    L.rows = m.take((size_t)T * sizeof(int32_t));
    L.table_bytes = evi_first_occurrence_workspace_bytes(T, Q);
    L.table = m.take(L.table_bytes);
    L.total = m.total;
    return L;
}

template <class RowT>
static void launch_cand_score(hipStream_t st, int64_t waves, const float* q, int D, const void* idx, const float* row_scale,
                              const int64_t* keys, const int64_t* seg_ptr, const int32_t* uniq_pos, const int32_t* count,
                              const int32_t* tile_pre, int Q, float* scores, int32_t* rows) {
    launch_timed(kTimeCosineScore, k_cand_score<RowT>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, q, D,
                 static_cast<const RowT*>(idx), row_scale, keys, seg_ptr, uniq_pos, count, tile_pre, Q, scores, rows);
}

}  // namespace evi

extern "C" size_t evi_cosine_topk_candidates_workspace_bytes(int Q, int64_t T, int k) {
    if (Q < 0 || T < 0 || k <= 0) return 0;
    return cand_layout(Q, T).total;
}

extern "C" int evi_cosine_topk_candidates(const float* q, int Q, const void* idx, int kind, int64_t N, int D, const float* row_scale,
                                          const int64_t* cand_ids, const int64_t* cand_ptr, int64_t T, int k, int64_t row_id_base,
                                          int64_t id_limit, float* out_score, int64_t* out_index, int32_t* status, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    EVI_REQUIRE(kind >= kIdxF32 && kind <= kIdxFp8Mfma, "evi_cosine_topk_candidates: kind must be 0 (f32), 1 (f16), 2 (e4m3 widened) "
                "or 3 (e4m3 native MFMA), got %d", kind);
    EVI_REQUIRE(Q >= 0 && N >= 0 && T >= 0, "evi_cosine_topk_candidates: need Q >= 0, N >= 0 and T >= 0, got Q=%d N=%lld T=%lld", Q,
                (long long)N, (long long)T);
    EVI_REQUIRE(N < (int64_t)0x7FFFFFFF, "evi_cosine_topk_candidates: a shard holds at most 2^31-1 rows, got %lld", (long long)N);
    EVI_REQUIRE(T / 16 + Q < (int64_t)0x7FFFFFFF - 1, "evi_cosine_topk_candidates: T / 16 + Q must stay below 2^31, got T=%lld Q=%d",
                (long long)T, Q);
    EVI_REQUIRE(T <= (int64_t)0x7FFFFFFF, "evi_cosine_topk_candidates: at most 2^31-1 list entries per call, got %lld", (long long)T);
    EVI_REQUIRE(k >= 1 && k <= EVI_TOPK_MAX_K, "evi_cosine_topk_candidates: k must be in [1, %d], got %d", EVI_TOPK_MAX_K, k);
    if (D < 16 || D % 16 != 0 || D > 1280)
        return fail(EVI_ERR_UNSUPPORTED, "evi_cosine_topk_candidates: D must be a multiple of 16 in [16, 1280], got %d", D);
    if (kind == kIdxF16 && D % 32 != 0)
        return fail(EVI_ERR_UNSUPPORTED, "evi_cosine_topk_candidates: an f16 index needs D to be a multiple of 32, got %d", D);
    if (kind >= kIdxFp8Widen && D % 64 != 0)
        return fail(EVI_ERR_UNSUPPORTED, "evi_cosine_topk_candidates: an e4m3 index needs D to be a multiple of 64, got %d", D);
    EVI_REQUIRE(kind < kIdxFp8Widen || row_scale,
                "evi_cosine_topk_candidates: row_scale (the per-row dequantisation scale) is required for an e4m3 index");
    if (Q == 0) return EVI_OK;
    EVI_REQUIRE(q && cand_ptr && out_score && out_index && workspace && (T == 0 || cand_ids) && (N == 0 || idx),
                "evi_cosine_topk_candidates: null pointer");
    const CandLayout L = cand_layout(Q, T);
    if (workspace_bytes < L.total)
        return fail(EVI_ERR_NOMEM, "evi_cosine_topk_candidates: workspace %zu B < %zu B", workspace_bytes, L.total);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(workspace);
    int64_t* seg_ptr = reinterpret_cast<int64_t*>(base + L.seg_ptr);
    int64_t* keys = reinterpret_cast<int64_t*>(base + L.keys);
    uint8_t* drop = reinterpret_cast<uint8_t*>(base + L.drop);
    int32_t* first = reinterpret_cast<int32_t*>(base + L.first);
    int32_t* rank = reinterpret_cast<int32_t*>(base + L.rank);
    int32_t* uniq_pos = reinterpret_cast<int32_t*>(base + L.uniq_pos);
    int32_t* count = reinterpret_cast<int32_t*>(base + L.count);
    int32_t* tile_pre = reinterpret_cast<int32_t*>(base + L.tile_pre);
    float* scores = reinterpret_cast<float*>(base + L.scores);
    int32_t* rows = reinterpret_cast<int32_t*>(base + L.rows);

    hipLaunchKernelGGL(k_cand_ptr, dim3(1), dim3(kCandThreads), 0, st, cand_ptr, Q, T, seg_ptr, status);
    EVI_LAUNCH_CHECK();
    if (T > 0) {
        hipLaunchKernelGGL(k_cand_mark, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, cand_ids, T, N, row_id_base, id_limit, keys,
                           drop, status);
        EVI_LAUNCH_CHECK();
    }
    if (T == 0 || N == 0) {  // nothing to score: all padding
        hipLaunchKernelGGL(k_cand_select, dim3(Q), dim3(kSelectThreads), 0, st, scores, rows, seg_ptr, (const int32_t*)nullptr, k,
                           row_id_base, out_score, out_index);
        EVI_LAUNCH_CHECK();
        return EVI_OK;
    }
    int rc = evi_first_occurrence(keys, 1, T, seg_ptr, Q, drop, first, base + L.table, L.table_bytes, stream);
    if (rc != EVI_OK) return rc;
    rc = evi_first_seen_rank(first, T, seg_ptr, Q, nullptr, rank, count, uniq_pos, stream);
    if (rc != EVI_OK) return rc;
    hipLaunchKernelGGL(k_cand_tiles, dim3(1), dim3(kCandThreads), 0, st, count, Q, tile_pre);
    EVI_LAUNCH_CHECK();
    const int64_t waves = (T + 15) / 16 + Q;  // >= sum over queries of ceil(count / 16)
    switch ((IndexKind)kind) {
        case kIdxF32: launch_cand_score<float>(st, waves, q, D, idx, row_scale, keys, seg_ptr, uniq_pos, count, tile_pre, Q, scores, rows); break;
        case kIdxF16: launch_cand_score<_Float16>(st, waves, q, D, idx, row_scale, keys, seg_ptr, uniq_pos, count, tile_pre, Q, scores, rows); break;
        case kIdxFp8Widen: launch_cand_score<Fp8WidenRow>(st, waves, q, D, idx, row_scale, keys, seg_ptr, uniq_pos, count, tile_pre, Q, scores, rows); break;
        default: launch_cand_score<Fp8MfmaRow>(st, waves, q, D, idx, row_scale, keys, seg_ptr, uniq_pos, count, tile_pre, Q, scores, rows); break;
    }
    EVI_LAUNCH_CHECK();
    launch_timed(kTimeSelect, k_cand_select, dim3(Q), dim3(kSelectThreads), 0, st, scores, rows, seg_ptr, count, k, row_id_base,
                 out_score, out_index);
    EVI_LAUNCH_CHECK();
    return EVI_OK;
}
