// lmrs_score.h — launch interface of the scoring reduction (lmrs_score.hip): per-row argmax and log-softmax of a target over
// blocks of logits, for lmrs_score_tokens (include/lmrs_hip.h), and the k first candidates of every row, for lmrs_score_tokens_topk / lmrs_forward_topk.
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

// The k first candidates of every row of the same kind of block, in this order: all `vocab` entries take part (zero tail included); the larger
// value first, -0.0 == +0.0; equal values by ascending index; a NaN after every number, NaNs by ascending index - but a NaN at index 0 takes
// rank 0, so that rank 0 is out_idx of launch_score_rows in every case.  1 <= k <= kTopkMax, k <= vocab.
//   out_idx[r * k + j] = the rank-j index; out_val[r * k + j] = its f32 logit - or, with `part` (the chunk summaries launch_score_rows left for
//   the SAME rows), (double)l - m - log(sum) rounded once to float, m and sum exactly those of that row's out_lp;
//   out_rank[r] (r < n_tgt, tgt as in ScoreArgs; optional) = the number of candidates that precede entry tgt[r]: exact for any rank.
// cand: rows * score_chunks(vocab) * k keys, cnt: rows * score_chunks(vocab) counts (scratch between the two launches).  The chunking is that
// of the scores and no result depends on the order in which lanes or workgroups arrive: a row gives the same bits in any launch.
constexpr int kTopkMax = 256;
struct TopkArgs {
    const float* logits; int ld, written, vocab, rows, k;
    const uint32_t* tgt; int n_tgt;
    const ScorePart* part;
    unsigned long long* cand; uint32_t* cnt;
    uint32_t* out_idx; float* out_val; uint32_t* out_rank;
};
hipError_t launch_topk_rows(const TopkArgs& a, hipStream_t s);

// logits[r * ld + i] = 30 * (float)tanh((double)(logits[r * ld + i] / 30)) for r < rows, i < cols (cols <= ld): Gemma-2's soft-cap of the first
// `dim` logits (transformer.rs:375-381), the decode classifier epilogue's arithmetic over a block of rows
hipError_t launch_softcap_rows(float* logits, int ld, int cols, int rows, hipStream_t s);

// logits[r * ld + t] = -inf for r < rows with mask_of[r] >= 0 and every t < cols whose bit - bit (t & 31) of word (t >> 5) of mask row mask_of[r],
// `words` words a row of `bits` - is clear; nothing else is written and nothing of the block is read.  cols % 4 == 0, ld % 4 == 0, cols <= 32 * words,
// the block 16-byte aligned.  (lmrs_batch_set_masks: behind the soft-cap, in front of every sink)
hipError_t launch_mask_rows(float* logits, int ld, int cols, int rows, const uint32_t* bits, int words, const int* mask_of, hipStream_t s);

// ---- token automata on batch slots (lmrs_batch_automaton_create / lmrs_batch_attach_automaton): the mask of a slot follows the token it chose
// The tables on the device: class_of[vocab] (uint16_t), next[n_states][n_classes] - a state with kAutoFinalBit where that state is final, or kAutoDead -
// and masks[n_states][words] in lmrs_batch_set_masks' bit layout.
constexpr uint32_t kAutoDead = 0xFFFFFFFFu;                 // = LMRS_STATE_DEAD
constexpr uint32_t kAutoFinalBit = 0x80000000u;
// bits[q * words + w] for q < n_states, w < words = (vocab + 31) / 32: bit (t & 31) of word (t >> 5) set iff next[q * n_classes + class_of[t]] != kAutoDead;
// bits at and above vocab clear.  Every class_of entry is below n_classes (the caller checked).  Stores only, every word by one lane, no atomics.
hipError_t launch_automaton_masks(const uint16_t* class_of, const uint32_t* next, int vocab, uint32_t n_states, uint32_t n_classes, uint32_t* bits, hipStream_t s);
// One output row's automaton, in the order the classifier sees the rows: slot < 0 - none; else the tables of the automaton the slot is attached to.
// The slot's state is NOT in here: it is read on the device from the batch's state words (state[slot]), where launch_gen_advance leaves it.
struct AutoRow { const uint32_t* masks; const uint16_t* class_of; const uint32_t* next; uint32_t n_classes, n_states, vocab; int slot; };
// launch_mask_rows with the mask resolved on the device: row r < rows with of[r].slot >= 0 is masked under of[r].masks + state[of[r].slot] * words (a state
// word that is not below n_states: the row is left alone).  Same stores, one more dependent load per workgroup; same conditions on cols, ld and the block.
hipError_t launch_auto_mask_rows(float* logits, int ld, int cols, int rows, const AutoRow* of, const uint32_t* state, int words, hipStream_t s);

// ---- a batch's token record and the penalties over it (lmrs_batch_set_history / lmrs_batch_set_penalties)
constexpr uint32_t kTokenNone = 0xFFFFFFFFu;                // = LMRS_TOKEN_NONE: a position whose token is unknown, or an embedding row
constexpr int kPenaltyKeysMax = 8192;                       // the keys one workgroup sorts in LDS (32 KB): the clamp of seq_len
// hist[slot_of[r] * seq_len + pos[r]] = tok[r] for r < n_rows, kTokenNone where tok[r] has the stage bit of an embedding row (kRowFromStage); a row whose
// slot or position lies outside [0, n_slots) x [0, seq_len) writes nothing.  pos / tok are the columns of the pass's device table as they stand.
hipError_t launch_record_rows(uint32_t* hist, int seq_len, int n_slots, const int* pos, const uint32_t* tok, const int* slot_of, int n_rows, hipStream_t s);
// One output row's penalties, in the order the classifier sees the rows: slot < 0 - none; tab_row - the row of the pass's device table whose position is the row's
struct PenaltyRow { int slot; int tab_row; float repetition, presence, frequency; uint32_t out_from; };
// Row r < rows of the block with of[r].slot >= 0, at position p = pos[of[r].tab_row] (read on the device): over H = the entries of hist[slot][0 .. p] that are not
// kTokenNone, c_all[t] = occurrences of t, c_out[t] = those at positions >= out_from; for every t with c_all[t] > 0 and repetition != 1,
// l[t] = l[t] > 0 ? l[t] / repetition : l[t] * repetition; then for every t with c_out[t] > 0, l[t] = (l[t] - frequency * (float)c_out[t]) - presence - each
// operation one correctly rounded f32 operation, nothing contracted.  No other logit is read or written, each penalised one by exactly one thread, and the
// counts are integers: the result does not depend on scheduling.  max_n >= every row's p + 1, at most min(seq_len, kPenaltyKeysMax): sizes the launch's LDS.
hipError_t launch_penalty_rows(float* logits, int ld, int cols, int rows, const uint32_t* hist, int seq_len, const int* pos, const PenaltyRow* of, int max_n, hipStream_t s);

// ---- a batch slot's candidate filters (lmrs_batch_set_filters): top_k and min_gap over a row, behind the masks and in front of every sink
// One output row's filter, in the order the classifier sees the rows: slot < 0 - none; top_k 0 or >= cols - off; min_gap +inf - off
struct FilterRow { int slot; uint32_t top_k; float min_gap; };
// Row r < rows of the block with of[r].slot >= 0, over its first `cols` entries in the candidate order above (launch_topk_rows: the 64-bit keys of topk_key),
// m = the value of the first candidate:
//   1 <= top_k < cols: every entry that is not among the first top_k candidates becomes -inf (the k-th key is found exactly, ties at its value by index);
//   min_gap finite and m a number: thr = m - min_gap, one correctly rounded f32 subtraction; every entry with !(l >= thr) becomes -inf.
// Only -inf is stored, and never over a kept entry; the first candidate is always kept.  The counts are integer sums in LDS, nothing global is written but
// the row, and what is written depends on key values alone: a row gives the same bits in any launch.  One workgroup a row; rows <= 65535, cols <= ld.
hipError_t launch_filter_rows(float* logits, int ld, int cols, int rows, const FilterRow* of, hipStream_t s);

// ---- the step boundary of lmrs_batch_generate's device loop: one block per output row of the pass's table, in the order the classifier sees the rows
constexpr int kGenStopMax = 16;                             // = LMRS_STOP_MAX
constexpr int kGenRowsMax = 64;                             // one lane per row: a wide batch's rows
// live: the row still generates; done: tokens it has produced; budget: its max_new; finish: 0 budget / 1 stop (valid once live == 0); last: the token it
// chose last; out_at: where its outputs start in the call's output blocks (words); from_samp: its token is word 0 of its sampling result block, else idx[o]
struct GenRow { uint32_t live, done, budget, finish, last, out_at, from_samp, n_stop; uint32_t stop[kGenStopMax]; };
// Where the chosen tokens stand behind a pass: idx[o] (the reduction's sample_argmax) or the low word of samp[o * samp_ld] (launch_sample_rows' result blocks)
struct GenPick { const uint32_t* idx; const unsigned long long* samp; size_t samp_ld; };
// Output o < n_rows, live: t = its chosen token -> out[out_at + done]; done += 1; t in its stop set: live = 0, finish = 1; else done == budget: live = 0,
// finish = 0; else the table row behind it (sel[o]; sel null: row o) gets tok = t, pos += 1.  A row that is not live changes nothing: its table row stays, so
// the next pass computes the same row again.  *n_live = the rows still live.  One lane per row, plain stores.
// aut (null: no row of the pass has an automaton - the launch is the kernel it was without them): output o's automaton, state the batch's state words.  For a
// live row with one, q' = next[state[slot]][class_of[t]]; behind the stop test and in front of the budget's: q' final - live = 0, finish = 3 (kGenFinishFinal); a row
// that stays live stores q' in state[slot]; a row that ends leaves its state word alone (its recomputed last row is masked as it was; the host completes the walk).
constexpr uint32_t kGenFinishFinal = 3;                     // = LMRS_FINISH_FINAL (2 is launch_topp_rows' row without a candidate)
hipError_t launch_gen_advance(GenRow* st, int* pos, uint32_t* tok, const uint32_t* sel, GenPick pick, uint32_t* out, uint32_t* n_live, int n_rows, hipStream_t s,
                              const AutoRow* aut = nullptr, uint32_t* state = nullptr);
// In front of launch_gen_advance, for every live output o: lp_out[out_at + done] = (float)((double)l[t] - m - log(sum)) of row o of `logits` (ld floats a row,
// all `vocab` written), t the token launch_gen_advance is about to record, m and sum from the chunk summaries launch_score_rows left for the SAME rows in
// `part`: score_merge_kernel's arithmetic, one rounding to float.  One wave per row.
hipError_t launch_gen_logprobs(const GenRow* st, GenPick pick, const float* logits, int ld, int vocab, const ScorePart* part, float* lp_out, int n_rows, hipStream_t s);

}  // namespace lmrs
