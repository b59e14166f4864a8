// lmrs_score.h — launch interface of the scoring reduction (lmrs_score.hip): per-row argmax and log-softmax of a target over
// blocks of logits, for lmrs_score_tokens (include/lmrs_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace lmrs {

// One row's chunk summary: f32 maximum, first index of it (INT_MAX: no value in the chunk is a number), sum of exp(l - max) in double
struct ScorePart { float max; int idx; double sum; };

constexpr int kScoreChunk = 2048;                           // logits per workgroup of the first pass (256 lanes x 8)
__host__ __device__ inline int score_chunks(int vocab) { return (vocab + kScoreChunk - 1) / kScoreChunk; }

// rows x `vocab` logits, row r at logits + r * ld; columns [written, vocab) are never read and count as 0.0 (the classifier's unwritten tail).
// For row r: out_idx[r] = Sampler::sample_argmax (sampler.rs:29-41: first index of the maximum, a NaN at index 0 is never displaced);
// for r < n_tgt also out_lp[r] = (double)l[tgt[r]] - m - log(sum_i exp((double)l_i - m)), m = the f32 maximum.  part: rows * score_chunks(vocab).
// The chunking depends on `vocab` alone, so a row gives the same bits whatever the launch around it.
struct ScoreArgs {
    const float* logits; int ld, written, vocab, rows;
    const uint32_t* tgt; int n_tgt;
    ScorePart* part; double* out_lp; uint32_t* out_idx;
};
hipError_t launch_score_rows(const ScoreArgs& a, hipStream_t s);

// logits[r * ld + i] = 30 * (float)tanh((double)(logits[r * ld + i] / 30)) for r < rows, i < cols (cols <= ld): Gemma-2's soft-cap of the first
// `dim` logits (transformer.rs:375-381), the decode classifier epilogue's arithmetic over a block of rows
hipError_t launch_softcap_rows(float* logits, int ld, int cols, int rows, hipStream_t s);

}  // namespace lmrs
