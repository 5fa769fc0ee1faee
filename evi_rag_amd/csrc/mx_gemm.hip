// MXFP8 linear layer on gfx950's block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4):  y = x * W^T (+ bias).
//
// Format (the contract the tests pin bit for bit; tests/mx_oracle.py restates it on the CPU): every row of an operand is cut
// into blocks of 32 consecutive K elements.  For a block with amax = max|x| (read as f32), the scale exponent is
//   e = max(-127, ceil(log2(amax / 448)))  (amax > 0),   e = -127  (all zeros),
// computed exactly from the exponent and mantissa bits: the smallest power of two with amax / 2^e <= 448.  The scale byte is
// e + 127 (e8m0) and the elements are e4m3fn(x * 2^-e), round to nearest even, subnormals kept.  The OCP rule
// floor(log2 amax) - 8 puts block maxima in [256, 512) and saturates those above 448; this rule never saturates.
// A block holding NaN or +-inf gets scale 0xFF and NaN bytes, and every output that reads it is written as NaN.
//
// Lane maps of the 16x16x128 f8f6f4 form with e4m3 operands (settled on the device with one-hot operands and per-lane
// scales; tests/test_mx_gpu.py re-checks them with exact integer data).  Within one 128-deep K step, lane l (g = l >> 4)
// holds row (l & 15) at k = 16 g + j in bytes j = 0..15 and at k = 64 + 16 g + j in bytes 16 + j: its 32 bytes are HALVES
// OF TWO MX blocks, not one.  The scale operand does follow the blocks: lane l supplies the scale byte of row (l & 15),
// block l >> 4 (k = 32 (l >> 4) .. + 31).  The output D[i][j] has j = lane & 15 and i = 4 * (lane >> 4) + r in register r.
// The weight is the A operand (i = output column n) and the activation the B operand (j = output row m), so a lane ends
// with four consecutive columns of one row of y: one 16-byte (f32) or 8-byte (bf16 / f16) store.
//
// Tiling: 128 (M) x 256 (N) output tile per 512-thread workgroup, K steps of 128 (one MFMA deep).  Eight waves as
// 2 (M) x 4 (N), each 64 x 64 = 4 x 4 MFMA tiles.  Activation: every thread loads one 32-element row block per K step with
// 16-byte loads one step ahead, finds its amax in registers, converts it and writes 32 bytes + its scale byte into the
// other half of a double-buffered LDS tile (16-byte chunks XOR-swizzled by row).  Weight: quantised once by
// evi_mx_pack_weight into fragment order, so each wave reads its weight fragments straight from global memory with
// 16-byte loads, one K step ahead, and one u32 per lane carries the scale bytes of its four 16-column tiles.
#include "common.hpp"

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <type_traits>

namespace evi {
namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

constexpr int kBM = 128, kBN = 256, kKS = 128;  // output tile, K step
constexpr int kThreads = 512;
constexpr int kGroupN = 64;                       // columns per packed weight group (one wave's N extent)

// ---- the format ------------------------------------------------------------------------------------------------------

// scale exponent of a block from the bits of its amax (sign cleared); amax_bits >= 0x7F800000 (non-finite) is handled by
// the caller
__device__ inline int mx_scale_exp(uint32_t amax_bits) {
    const int biased = (int)(amax_bits >> 23);
    if (biased == 0) return -127;  // zero or f32 subnormal: amax < 2^-126, so amax / 2^-127 < 2 <= 448
    const int E = biased - 127;
    const int e = (amax_bits & 0x7FFFFFu) > 0x600000u ? E - 7 : E - 8;  // mantissa above 1.75 (448 = 1.75 * 2^8)
    return e < -127 ? -127 : e;
}

// e4m3fn of a finite |v| <= 448 (the callers guarantee it), round to nearest even, subnormals kept
__device__ inline uint32_t e4m3_rne(float v) {
    const uint32_t u = __float_as_uint(v);
    const uint32_t s = (u >> 24) & 0x80u;
    const uint32_t a = u & 0x7FFFFFFFu;
    uint32_t q;
    if (a < 0x3C800000u) {  // below 2^-6, e4m3's smallest normal: a multiple of 2^-9 (8 = the smallest normal's code)
        q = (uint32_t)__builtin_rintf(__uint_as_float(a) * 512.0f);
    } else {                // keep 3 mantissa bits, round to nearest even; a carry moves into the exponent
        q = ((a + 0x7FFFFu + ((a >> 20) & 1u)) >> 20) - ((127u - 7u) << 3);
    }
    return s | q;
}

// four e4m3 bytes, element r in byte r.  v_cvt_pk_fp8_f32 (OCP e4m3 on gfx950, round to nearest even); EVI_MX_SOFT_CVT
// selects the integer restatement above instead
__device__ inline uint32_t e4m3_pack4(float a, float b, float c, float d) {
#ifdef EVI_MX_SOFT_CVT
    return e4m3_rne(a) | (e4m3_rne(b) << 8) | (e4m3_rne(c) << 16) | (e4m3_rne(d) << 24);
#else
    int r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
    return (uint32_t)r;
#endif
}

// Quantise one block of 32 f32 values: 8 u32 words of e4m3 bytes (element 4w + b in byte b of word w) and the scale
// byte.  Returns true when the block holds a NaN or an infinity.
__device__ inline bool mx_quantize_block(const float (&v)[32], uint32_t (&q)[8], uint32_t& scale) {
    uint32_t amax = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) amax = max(amax, __float_as_uint(v[i]) & 0x7FFFFFFFu);
    if (amax >= 0x7F800000u) {
#pragma unroll
        for (int w = 0; w < 8; ++w) q[w] = 0x7F7F7F7Fu;
        scale = 0xFFu;
        return true;
    }
    const int e = mx_scale_exp(amax);
    scale = (uint32_t)(e + 127);
    const float mul = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e, a normal f32 for e in [-127, 120]
#pragma unroll
    for (int w = 0; w < 8; ++w) q[w] = e4m3_pack4(v[4 * w] * mul, v[4 * w + 1] * mul, v[4 * w + 2] * mul, v[4 * w + 3] * mul);
    return false;
}

__device__ inline float to_f32(float x) { return x; }
__device__ inline float to_f32(__hip_bfloat16 x) { return __bfloat162float(x); }
__device__ inline float to_f32(__half x) { return __half2float(x); }

// the 32 elements of one block (16-byte loads when VEC: the block's address and the row stride are 16-byte aligned)
template <typename T, bool VEC>
__device__ inline void load_block(const T* __restrict__ p, float (&v)[32]) {
    if constexpr (VEC && sizeof(T) == 4) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(p + 4 * c);
            v[4 * c] = t[0]; v[4 * c + 1] = t[1]; v[4 * c + 2] = t[2]; v[4 * c + 3] = t[3];
        }
    } else if constexpr (VEC) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const u32x4 t = *reinterpret_cast<const u32x4*>(p + 8 * c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t w = t[j];
                if constexpr (std::is_same<T, __hip_bfloat16>::value) {
                    v[8 * c + 2 * j] = __uint_as_float(w << 16);
                    v[8 * c + 2 * j + 1] = __uint_as_float(w & 0xFFFF0000u);
                } else {
                    v[8 * c + 2 * j] = __half2float(__ushort_as_half((unsigned short)(w & 0xFFFFu)));
                    v[8 * c + 2 * j + 1] = __half2float(__ushort_as_half((unsigned short)(w >> 16)));
                }
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 32; ++i) v[i] = to_f32(p[i]);
    }
}

// ---- standalone row quantiser ----------------------------------------------------------------------------------------

template <typename T>
__global__ void k_mx_quantize_rows(const T* __restrict__ x, int64_t M, int K, int64_t ldx, uint8_t* __restrict__ q,
                                   uint8_t* __restrict__ scale) {
    const int nb = K / 32;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * nb) return;
    const int64_t m = i / nb;
    const int b = (int)(i % nb);
    float v[32];
    load_block<T, false>(x + m * ldx + 32 * b, v);
    uint32_t w[8], s;
    mx_quantize_block(v, w, s);
    u32x4* dst = reinterpret_cast<u32x4*>(q + m * K + 32 * b);  // 32-byte aligned: K % 32 == 0
    dst[0] = u32x4{w[0], w[1], w[2], w[3]};
    dst[1] = u32x4{w[4], w[5], w[6], w[7]};
    scale[i] = (uint8_t)s;
}

// ---- packed weight ---------------------------------------------------------------------------------------------------
// Layout (private): G = ceil(N / 64) groups of 64 columns, S = ceil(K / 128) K steps.
//   bytes  [G][S][4 tiles][64 lanes][32 B]  lane l of tile t: row 64g + 16t + (l & 15); bytes 0..15 hold k = 128 s + 16 (l >> 4)
//                                           + j, bytes 16..31 k = 128 s + 64 + 16 (l >> 4) + j (the MFMA's operand map)
//   scales [G][S][64 lanes] u32             byte t = the scale of row 64g + 16t + (l & 15), K block 4s + (l >> 4)
//   flags  [G * 64] u8                      1 where the row holds a NaN or an infinity
// Rows >= N and blocks >= K / 32 are zero bytes with scale byte 0.

struct PackLayout {
    int64_t groups, steps, scale_off, flag_off, total;
};

inline PackLayout pack_layout(int N, int K) {
    PackLayout p;
    p.groups = (N + kGroupN - 1) / kGroupN;
    p.steps = (K + kKS - 1) / kKS;
    const int64_t bytes = p.groups * p.steps * 4 * 64 * 32;
    p.scale_off = bytes;
    p.flag_off = p.scale_off + (int64_t)align_up((size_t)(p.groups * p.steps * 64 * 4), 256);
    p.total = p.flag_off + (int64_t)align_up((size_t)(p.groups * kGroupN), 256);
    return p;
}

template <typename T>
__global__ void k_mx_pack_weight(const T* __restrict__ w, int N, int K, int64_t ldw, int64_t steps,
                                 uint8_t* __restrict__ packed, int64_t scale_off, int64_t flag_off) {
    // one thread per (padded row, padded block); the row flags follow from the scale bytes (k_mx_pack_flags)
    const int64_t nb_pad = steps * 4;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t rows = (N + kGroupN - 1) / kGroupN * (int64_t)kGroupN;
    if (i >= rows * nb_pad) return;
    const int n = (int)(i / nb_pad);
    const int b = (int)(i % nb_pad);
    uint32_t q[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s = 0;
    if (n < N && b < K / 32) {
        float v[32];
        load_block<T, false>(w + (int64_t)n * ldw + 32 * b, v);
        mx_quantize_block(v, q, s);
    }
    const int g = n / kGroupN, t = (n % kGroupN) / 16, kb = b % 4;
    const int64_t step = (int64_t)g * steps + b / 4;
    uint8_t* tile = packed + (step * 4 + t) * 64 * 32;
    // the block's two 16-byte halves are chunks c = 2 kb and 2 kb + 1 of the step: lane group c % 4, byte half c / 4
    const int c0 = 2 * kb, c1 = 2 * kb + 1;
    *reinterpret_cast<u32x4*>(tile + ((n % 16) + 16 * (c0 % 4)) * 32 + 16 * (c0 / 4)) = u32x4{q[0], q[1], q[2], q[3]};
    *reinterpret_cast<u32x4*>(tile + ((n % 16) + 16 * (c1 % 4)) * 32 + 16 * (c1 / 4)) = u32x4{q[4], q[5], q[6], q[7]};
    packed[scale_off + (step * 64 + (n % 16) + 16 * kb) * 4 + t] = (uint8_t)s;
}

// the row flags, read back from the scale bytes the pack kernel wrote (0xFF marks a non-finite block)
__global__ void k_mx_pack_flags(int64_t rows, int64_t steps, uint8_t* __restrict__ packed, int64_t scale_off,
                                int64_t flag_off) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= rows) return;
    const int64_t g = n / kGroupN;
    const int t = (int)((n % kGroupN) / 16), r = (int)(n % 16);
    uint8_t bad = 0;
    for (int64_t b = 0; b < steps * 4; ++b) {
        const int64_t step = g * steps + b / 4;
        const int lane = r + 16 * (int)(b % 4);
        bad |= packed[scale_off + (step * 64 + lane) * 4 + t] == 0xFFu;
    }
    packed[flag_off + n] = bad;
}

// ---- the GEMM --------------------------------------------------------------------------------------------------------

template <typename TY>
__device__ inline void store4(TY* p, f32x4 v, bool vec, int cnt) {
    if constexpr (sizeof(TY) == 4) {
        if (vec) { *reinterpret_cast<f32x4*>(p) = v; return; }
    } else {
        if (vec) {
            u16x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const TY c = (TY)v[r];
                h[r] = *reinterpret_cast<const unsigned short*>(&c);
            }
            *reinterpret_cast<u16x4*>(p) = h;
            return;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (r < cnt) p[r] = (TY)v[r];
}

template <typename TX, typename TY, bool VEC>
__global__ __launch_bounds__(kThreads) void k_mx_linear(const TX* __restrict__ x, int64_t M, int K, int64_t ldx,
                                                        const uint8_t* __restrict__ packed, int N, int64_t steps,
                                                        int64_t scale_off, int64_t flag_off, const float* __restrict__ bias,
                                                        TY* __restrict__ y, int64_t ldy, bool vec_y) {
    // A tile: [2 buffers][128 rows][8 chunks of 16 B], chunk c of row r at slot c ^ (r & 7); scale bytes
    // [2][4 K blocks][2 wave rows][16 rows][4 M tiles] so that a lane reads its four tiles' scales as one u32
    __shared__ u32x4 sx[2][kBM * 8];
    __shared__ uint32_t ssc[2][4 * 2 * 16];
    __shared__ uint32_t srow_bad[kBM];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 2, wn = wave & 3;
    const int tiles_n = (N + kBN - 1) / kBN;
    // XCD-aware tile order (as gemm_bf16x3.hip): workgroups are dealt round-robin over the 8 XCDs, so give each XCD a
    // contiguous run of tiles; the n-tiles of one row panel are consecutive and share the activation rows in that L2
    const unsigned nwg = gridDim.x, nwg8 = nwg - nwg % 8;
    const unsigned tile = blockIdx.x < nwg8 ? (blockIdx.x % 8) * (nwg8 / 8) + blockIdx.x / 8 : blockIdx.x;
    const int64_t m0 = (int64_t)(tile / tiles_n) * kBM;
    const int n0 = (int)(tile % tiles_n) * kBN;

    // activation staging: thread -> (row ar, block ab) of every K step
    const int ar = tid >> 2, ab = tid & 3;
    const bool row_ok = m0 + ar < M;
    const TX* xrow = x + (row_ok ? (m0 + ar) * ldx : 0);
    const int nblk = K / 32;
    float av[32];
    uint32_t bad_row = 0;
    auto load_a = [&](int64_t s) {
        const int64_t b = s * 4 + ab;
        if (row_ok && b < nblk) {
            load_block<TX, VEC>(xrow + 32 * b, av);
        } else {
#pragma unroll
            for (int i = 0; i < 32; ++i) av[i] = 0.f;
        }
    };
    auto store_a = [&](int buf) {
        uint32_t q[8], s;
        bad_row |= mx_quantize_block(av, q, s) ? 1u : 0u;
        const int sw = ar & 7;
        sx[buf][ar * 8 + ((2 * ab) ^ sw)] = u32x4{q[0], q[1], q[2], q[3]};
        sx[buf][ar * 8 + ((2 * ab + 1) ^ sw)] = u32x4{q[4], q[5], q[6], q[7]};
        reinterpret_cast<uint8_t*>(ssc[buf])[((ab * 2 + (ar >> 6)) * 16 + (ar & 15)) * 4 + ((ar >> 4) & 3)] = (uint8_t)s;
    };

    // weight fragments: this wave's 64-column group, straight from the packed image
    const int64_t g = (n0 >> 6) + wn;
    const bool g_ok = g * kGroupN < N;
    const uint8_t* wbase = packed + (g_ok ? g : 0) * steps * (4 * 64 * 32) + lane * 32;
    const uint32_t* wsc = reinterpret_cast<const uint32_t*>(packed + scale_off) + (g_ok ? g : 0) * steps * 64 + lane;
    i32x8 wf[4], wf_next[4];
    uint32_t ws = 0, ws_next = 0;
    auto load_w = [&](int64_t s, i32x8 (&f)[4], uint32_t& sc) {
        if (!g_ok) return;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const u32x4* p = reinterpret_cast<const u32x4*>(wbase + (s * 4 + t) * (64 * 32));
            const u32x4 lo = p[0], hi = p[1];
            f[t] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        }
        sc = wsc[s * 64];
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!g_ok) {
#pragma unroll
        for (int t = 0; t < 4; ++t) wf[t] = wf_next[t] = i32x8{0, 0, 0, 0, 0, 0, 0, 0};
    }

    load_a(0);
    load_w(0, wf, ws);
    store_a(0);
    __syncthreads();
    for (int64_t s = 0; s < steps; ++s) {
        const int buf = (int)(s & 1);
        const bool more = s + 1 < steps;
        if (more) {
            load_a(s + 1);
            load_w(s + 1, wf_next, ws_next);
        }
        if (g_ok) {
            const uint32_t xs = ssc[buf][(((lane >> 4) * 2 + wm) * 16) + (lane & 15)];
#pragma unroll
            for (int i = 0; i < 4; ++i) {  // M tile i: rows wm * 64 + 16 i + (lane & 15)
                const int r = wm * 64 + 16 * i + (lane & 15);
                const int c = lane >> 4;  // 16-byte chunks c (k = 16 c ..) and 4 + c (k = 64 + 16 c ..): the lane map above
                const u32x4 lo = sx[buf][r * 8 + (c ^ (r & 7))];
                const u32x4 hi = sx[buf][r * 8 + ((c + 4) ^ (r & 7))];
                const i32x8 xf = {(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3],
                                  (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
                const int xsi = (int)((xs >> (8 * i)) & 0xFFu);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                        wf[j], xf, acc[i][j], 0, 0, 0, (int)((ws >> (8 * j)) & 0xFFu), 0, xsi);
            }
        }
        if (more) {
            store_a(buf ^ 1);  // that buffer was last read in step s - 1, before the barrier that ended it
#pragma unroll
            for (int t = 0; t < 4; ++t) wf[t] = wf_next[t];
            ws = ws_next;
        }
        __syncthreads();
    }

    // rows that read a non-finite activation block
    if (ab == 0) srow_bad[ar] = 0;
    __syncthreads();
    if (bad_row) srow_bad[ar] = 1;
    __syncthreads();
    if (!g_ok) return;

    const uint8_t* col_bad = packed + flag_off;
    const float qnan = __uint_as_float(0x7FC00000u);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + 16 * j + 4 * (lane >> 4);
        if (n >= N) continue;
        const int cnt = N - n < 4 ? N - n : 4;
        f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
        uint32_t cb = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r < cnt) {
                if (bias) b4[r] = bias[n + r];
                cb |= (uint32_t)col_bad[n + r] << r;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rl = wm * 64 + 16 * i + (lane & 15);
            const int64_t m = m0 + rl;
            if (m >= M) continue;
            f32x4 v = acc[i][j] + b4;
            const bool rb = srow_bad[rl] != 0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (rb || ((cb >> r) & 1u)) v[r] = qnan;
            store4<TY>(y + m * ldy + n, v, vec_y && cnt == 4, cnt);
        }
    }
}

template <typename TX, typename TY>
void launch_linear(const void* x, int64_t M, int K, int64_t ldx, const uint8_t* packed, int N, const PackLayout& p,
                   const float* bias, void* y, int64_t ldy, hipStream_t st) {
    const int64_t tiles = (M + kBM - 1) / kBM * ((N + kBN - 1) / kBN);
    const bool vec_x = ((uintptr_t)x % 16 == 0) && ((ldx * (int64_t)sizeof(TX)) % 16 == 0);
    const bool vec_y = ((uintptr_t)y % (4 * sizeof(TY)) == 0) && ((ldy * (int64_t)sizeof(TY)) % (4 * sizeof(TY)) == 0);
    auto kern = vec_x ? k_mx_linear<TX, TY, true> : k_mx_linear<TX, TY, false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(kThreads), 0, st, static_cast<const TX*>(x), M, K, ldx, packed, N,
                       p.steps, p.scale_off, p.flag_off, bias, static_cast<TY*>(y), ldy, vec_y);
}

template <typename TX>
void launch_linear_y(int y_dtype, const void* x, int64_t M, int K, int64_t ldx, const uint8_t* packed, int N,
                     const PackLayout& p, const float* bias, void* y, int64_t ldy, hipStream_t st) {
    if (y_dtype == 0) launch_linear<TX, float>(x, M, K, ldx, packed, N, p, bias, y, ldy, st);
    else if (y_dtype == 1) launch_linear<TX, __half>(x, M, K, ldx, packed, N, p, bias, y, ldy, st);
    else launch_linear<TX, __hip_bfloat16>(x, M, K, ldx, packed, N, p, bias, y, ldy, st);
}

}  // namespace
}  // namespace evi

using namespace evi;

extern "C" int evi_mx_quantize_rows(const void* x, int dtype_code, int64_t M, int K, int64_t ldx, uint8_t* out_e4m3,
                                    uint8_t* out_scale, void* stream) {
    EVI_REQUIRE(dtype_code >= 0 && dtype_code <= 2, "evi_mx_quantize_rows: dtype_code must be 0 (f32), 1 (f16) or 2 (bf16), got %d",
                dtype_code);
    EVI_REQUIRE(M >= 0 && K > 0, "evi_mx_quantize_rows: bad shape M=%lld K=%d", (long long)M, K);
    EVI_REQUIRE(K % 32 == 0, "evi_mx_quantize_rows: K=%d is not a multiple of the 32-element MX block", K);
    EVI_REQUIRE(ldx >= K, "evi_mx_quantize_rows: ldx=%lld < K=%d", (long long)ldx, K);
    if (M == 0) return EVI_OK;
    EVI_REQUIRE(x && out_e4m3 && out_scale, "evi_mx_quantize_rows: null pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t n = M * (K / 32);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (dtype_code == 0)
        hipLaunchKernelGGL(k_mx_quantize_rows<float>, grid, block, 0, st, static_cast<const float*>(x), M, K, ldx, out_e4m3, out_scale);
    else if (dtype_code == 1)
        hipLaunchKernelGGL(k_mx_quantize_rows<__half>, grid, block, 0, st, static_cast<const __half*>(x), M, K, ldx, out_e4m3, out_scale);
    else
        hipLaunchKernelGGL(k_mx_quantize_rows<__hip_bfloat16>, grid, block, 0, st, static_cast<const __hip_bfloat16*>(x), M, K, ldx,
                           out_e4m3, out_scale);
    EVI_LAUNCH_CHECK();
    return EVI_OK;
}

extern "C" size_t evi_mx_pack_weight_bytes(int N, int K) {
    if (N < 1 || K < 32 || K % 32 != 0) return 0;
    return (size_t)pack_layout(N, K).total;
}

extern "C" int evi_mx_pack_weight(const void* w, int dtype_code, int N, int K, int64_t ldw, uint8_t* packed, void* stream) {
    EVI_REQUIRE(dtype_code >= 0 && dtype_code <= 2, "evi_mx_pack_weight: dtype_code must be 0 (f32), 1 (f16) or 2 (bf16), got %d",
                dtype_code);
    EVI_REQUIRE(N >= 1 && K > 0, "evi_mx_pack_weight: bad shape N=%d K=%d", N, K);
    EVI_REQUIRE(K % 32 == 0, "evi_mx_pack_weight: K=%d is not a multiple of the 32-element MX block", K);
    EVI_REQUIRE(ldw >= K, "evi_mx_pack_weight: ldw=%lld < K=%d", (long long)ldw, K);
    EVI_REQUIRE(w && packed, "evi_mx_pack_weight: null pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const PackLayout p = pack_layout(N, K);
    const int64_t rows = p.groups * kGroupN;
    const int64_t n = rows * p.steps * 4;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (dtype_code == 0)
        hipLaunchKernelGGL(k_mx_pack_weight<float>, grid, block, 0, st, static_cast<const float*>(w), N, K, ldw, p.steps, packed,
                           p.scale_off, p.flag_off);
    else if (dtype_code == 1)
        hipLaunchKernelGGL(k_mx_pack_weight<__half>, grid, block, 0, st, static_cast<const __half*>(w), N, K, ldw, p.steps, packed,
                           p.scale_off, p.flag_off);
    else
        hipLaunchKernelGGL(k_mx_pack_weight<__hip_bfloat16>, grid, block, 0, st, static_cast<const __hip_bfloat16*>(w), N, K, ldw,
                           p.steps, packed, p.scale_off, p.flag_off);
    hipLaunchKernelGGL(k_mx_pack_flags, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, rows, p.steps, packed, p.scale_off,
                       p.flag_off);
    EVI_LAUNCH_CHECK();
    return EVI_OK;
}

extern "C" int evi_mx_linear(const void* x, int x_dtype_code, int64_t M, int K, int64_t ldx, const uint8_t* packed, int N,
                             const float* bias_or_null, void* y, int y_dtype_code, int64_t ldy, void* stream) {
    EVI_REQUIRE(x_dtype_code >= 0 && x_dtype_code <= 2, "evi_mx_linear: x_dtype_code must be 0 (f32), 1 (f16) or 2 (bf16), got %d",
                x_dtype_code);
    EVI_REQUIRE(y_dtype_code >= 0 && y_dtype_code <= 2, "evi_mx_linear: y_dtype_code must be 0 (f32), 1 (f16) or 2 (bf16), got %d",
                y_dtype_code);
    EVI_REQUIRE(M >= 0 && K > 0 && N >= 1, "evi_mx_linear: bad shape M=%lld K=%d N=%d", (long long)M, K, N);
    EVI_REQUIRE(K % 32 == 0, "evi_mx_linear: K=%d is not a multiple of the 32-element MX block", K);
    EVI_REQUIRE(ldx >= K && ldy >= N, "evi_mx_linear: ldx=%lld must be >= K=%d and ldy=%lld >= N=%d", (long long)ldx, K,
                (long long)ldy, N);
    if (M == 0) return EVI_OK;
    EVI_REQUIRE(x && packed && y, "evi_mx_linear: null pointer");
    EVI_REQUIRE((M + kBM - 1) / kBM * ((N + kBN - 1) / kBN) < (int64_t)0x7FFFFFFF, "evi_mx_linear: too many tiles (M=%lld N=%d)",
                (long long)M, N);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const PackLayout p = pack_layout(N, K);
    const uint8_t* pk = packed;
    if (x_dtype_code == 0) launch_linear_y<float>(y_dtype_code, x, M, K, ldx, pk, N, p, bias_or_null, y, ldy, st);
    else if (x_dtype_code == 1) launch_linear_y<__half>(y_dtype_code, x, M, K, ldx, pk, N, p, bias_or_null, y, ldy, st);
    else launch_linear_y<__hip_bfloat16>(y_dtype_code, x, M, K, ldx, pk, N, p, bias_or_null, y, ldy, st);
    EVI_LAUNCH_CHECK();
    return EVI_OK;
}
