// lmrs_score.hip — the reduction behind lmrs_score_tokens (include/lmrs_hip.h): over each row of a [tokens][vocab] block of logits, the
// first index of the f32 maximum (Sampler::sample_argmax, sampler.rs:29-41) and the log-softmax of a target token, in double.
//
// Two launches.  score_chunk_kernel: one workgroup of 256 lanes per 2048 logits of a row - two float4 loads per lane, the values stay in
// registers - forms the chunk's maximum and its first index, then sum exp((double)l - chunk max) over the chunk: one pass over HBM.
// score_merge_kernel: one wave per row merges the chunk summaries (maximum, first index, sum_c s_c * exp(max_c - max)) and forms
// l[y] - max - log(sum).  Llama's 128 256 logits are 63 workgroups per row: one token alone spreads over a quarter of the chip's CUs,
// 512 tokens over 32 k workgroups.  The rescaled sum differs from a direct sum of exp(l - max) by a few double ulps, far below the f32
// rounding of the result.  The summation order depends on the vocabulary size alone: a row gives the same bits in any launch.
//
// softcap_rows_kernel: Gemma-2's soft-cap of the first `dim` logits of every row of the block, between the batched classifier GEMM and the
// reduction (the decode classifier applies it in its epilogue).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "lmrs_score.h"

namespace lmrs {
namespace {

constexpr int kLanes = 256;
constexpr int kPerLane = kScoreChunk / kLanes;          // 8: two float4
static_assert(kPerLane == 8, "a lane holds two float4 of its chunk");

// (value, index) pairs: the larger value wins, equal values -> the lower index (the first maximum).  No NaN reaches these.
__device__ __forceinline__ void take_max(float& m, int& i, float om, int oi) {
    if (om > m || (om == m && oi < i)) { m = om; i = oi; }
}
__device__ __forceinline__ void wave_max(float& m, int& i) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) take_max(m, i, __shfl_xor(m, off), __shfl_xor(i, off));
}
// butterfly: every lane ends with the same sum (a + b == b + a), the order fixed by the lane numbering
__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

// grid (chunks of the row, rows).  VEC: rows start 16-byte aligned (ld % 4 == 0): float4 loads wherever four written values are whole
template <bool VEC>
__global__ __launch_bounds__(kLanes) void score_chunk_kernel(const ScoreArgs a) {
    __shared__ float s_max[kLanes / 64];
    __shared__ int s_idx[kLanes / 64];
    __shared__ double s_sum[kLanes / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = a.logits + (size_t)blockIdx.y * a.ld;
    const int c0 = blockIdx.x * kScoreChunk;
    float v[kPerLane];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i0 = c0 + 4 * (tid + k * kLanes);
        if (VEC && i0 + 3 < a.written) {
            const float4 f = *reinterpret_cast<const float4*>(row + i0);
            v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * k + j] = i0 + j < a.written ? row[i0 + j] : 0.0f;   // (past `vocab`: masked below)
        }
    }
    // the lane's first maximum (its indices ascend), NaNs skipped; then the workgroup's
    float m = -INFINITY; int mi = INT_MAX;
#pragma unroll
    for (int e = 0; e < kPerLane; ++e) {
        const int i = c0 + 4 * (tid + (e >> 2) * kLanes) + (e & 3);
        if (i < a.vocab && v[e] == v[e] && (v[e] > m || mi == INT_MAX)) { m = v[e]; mi = i; }
    }
    wave_max(m, mi);
    if (lane == 0) { s_max[wave] = m; s_idx[wave] = mi; }
    __syncthreads();
    m = s_max[0]; mi = s_idx[0];
#pragma unroll
    for (int w = 1; w < kLanes / 64; ++w) take_max(m, mi, s_max[w], s_idx[w]);
    // sum of exp(l - chunk max) in double (a chunk of -inf / NaN only: 0)
    double s = 0.0;
    if (m != -INFINITY) {
        const double md = (double)m;
#pragma unroll
        for (int e = 0; e < kPerLane; ++e) {
            const int i = c0 + 4 * (tid + (e >> 2) * kLanes) + (e & 3);
            if (i < a.vocab) s += exp((double)v[e] - md);
        }
    }
    s = wave_sum(s);
    if (lane == 0) s_sum[wave] = s;
    __syncthreads();
    if (tid == 0) {
        ScorePart p; p.max = m; p.idx = mi; p.sum = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        a.part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = p;
    }
}

// one wave per row (four rows per workgroup)
__global__ __launch_bounds__(kLanes) void score_merge_kernel(const ScoreArgs a) {
    const int r = blockIdx.x * (kLanes / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= a.rows) return;                                                // (wave-uniform)
    const int S = score_chunks(a.vocab);
    const ScorePart* pp = a.part + (size_t)r * S;
    float m = -INFINITY; int mi = INT_MAX;
    for (int c = lane; c < S; c += 64) take_max(m, mi, pp[c].max, pp[c].idx);
    wave_max(m, mi);
    const double md = (double)m;
    double s = 0.0;
    for (int c = lane; c < S; c += 64) {
        const ScorePart q = pp[c];
        if (q.max != -INFINITY) s += q.sum * exp((double)q.max - md);
    }
    s = wave_sum(s);
    if (lane == 0) {
        const float* row = a.logits + (size_t)r * a.ld;
        const float l0 = a.written > 0 ? row[0] : 0.0f;
        a.out_idx[r] = l0 != l0 || mi == INT_MAX ? 0u : (uint32_t)mi;     // a NaN at index 0 is never displaced (strict `>` from index 0)
        if (r < a.n_tgt) {
            const uint32_t y = a.tgt[r];
            const float ly = y < (uint32_t)a.written ? row[y] : 0.0f;
            a.out_lp[r] = (double)ly - md - log(s);
        }
    }
}

// Gemma-2's soft-cap of the first `cols` logits (transformer.rs:375-381) over a block of rows: l / 30, (float)tanh((double)l), * 30 - the three
// roundings of the decode classifier's epilogue (EPI_CLS, lmrs_kernels.hip) with the same device tanh, so a row carries the decode step's bits.
// grid (ceil(cols / 256), rows)
__global__ __launch_bounds__(kLanes) void softcap_rows_kernel(float* logits, int ld, int cols) {
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= cols) return;
    float* p = logits + (size_t)blockIdx.y * ld + i;
    float v = *p;
    v = v / 30.0f;
    v = (float)tanh((double)v);
    v = v * 30.0f;
    *p = v;
}

}  // namespace

hipError_t launch_softcap_rows(float* logits, int ld, int cols, int rows, hipStream_t s) {
    if (!logits || rows <= 0 || rows > 65535 || cols <= 0 || cols > ld) return hipErrorInvalidValue;
    hipLaunchKernelGGL(softcap_rows_kernel, dim3((cols + kLanes - 1) / kLanes, rows), dim3(kLanes), 0, s, logits, ld, cols);
    return hipGetLastError();
}

hipError_t launch_score_rows(const ScoreArgs& a, hipStream_t s) {
    if (a.rows <= 0 || a.rows > 65535 || a.vocab <= 0 || a.written < 0 || a.written > a.vocab || a.ld < a.written || !a.part || !a.out_idx ||
        (a.n_tgt > 0 && (!a.tgt || !a.out_lp)))
        return hipErrorInvalidValue;
    const dim3 grid(score_chunks(a.vocab), a.rows);
    if (a.ld % 4 == 0 && (reinterpret_cast<uintptr_t>(a.logits) & 15) == 0) hipLaunchKernelGGL(score_chunk_kernel<true>, grid, dim3(kLanes), 0, s, a);
    else hipLaunchKernelGGL(score_chunk_kernel<false>, grid, dim3(kLanes), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(score_merge_kernel, dim3((a.rows + kLanes / 64 - 1) / (kLanes / 64)), dim3(kLanes), 0, s, a);
    return hipGetLastError();
}

}  // namespace lmrs
