/*
 * lmrs_hip.h — C ABI of the MI355X-native decode hot path for lm.rs models.
 *
 * This is the drop-in boundary: every entry point replaces one
 * member of the public surface of `lmrs::transformer::Transformer`
 * (reference src/transformer.rs) or one of the L2 free functions in
 * src/functional.rs / src/quantization.rs.  The reference has no FFI of its own,
 * so the signatures below are what a Rust `extern "C"` block would bind (the
 * binding itself is shown in INTEGRATION.md).  Plain pointers and sizes only.
 *
 * The same prototypes, with the prefix `lmrs_ref_` instead of `lmrs_`, are
 * implemented by the CPU oracle (oracle/lmrs_oracle.c).  The oracle is test
 * infrastructure; nothing in this library calls it.
 *
 * Conventions
 *   - every function returning int: 0 = ok, <0 = error (text via lmrs_last_error()).
 *     The reference panics on error (assert!/expect); a Rust shim turns !=0 into panic!.
 *   - a context is NOT thread-safe (reference: `&mut self`); several contexts may coexist.
 *   - all host pointers are caller-owned unless stated.
 */
#ifndef LMRS_HIP_H
#define LMRS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lmrs_ctx lmrs_ctx;

/* Mirror of TransformerArgs (reference src/transformer.rs:57-74), natural C layout
 * (the on-disk struct is packed; see lmrs_create).  seq_len is already clamped to
 * 8192 as the reference does (src/transformer.rs:158-160). */
typedef struct lmrs_args {
    uint32_t dim, hidden_dim, n_layers, n_heads, head_size, n_kv_heads, vocab_size, seq_len;
    float    rms_norm_eps, rope_theta;
    uint8_t  q_type;      /* 0 None, 1 Q8_0, 2 Q4_0      (src/quantization.rs:1-6)  */
    uint8_t  model_type;  /* 0 GEMMA, 1 LLAMA, 2 PHI      (src/transformer.rs:50-55) */
    uint8_t  multimodal;
    uint8_t  _pad;
    uint32_t group_size;
} lmrs_args;

enum { LMRS_Q_NONE = 0, LMRS_Q8_0 = 1, LMRS_Q4_0 = 2 };
enum { LMRS_GEMMA = 0, LMRS_LLAMA = 1, LMRS_PHI = 2 };

/* ---- Transformer::new  (src/transformer.rs:134-314) -------------------------------
 * Parses an LMRS v4 image (`file`,`len` = the mmap the reference hands to
 * Transformer::new), uploads the weights to HBM on HIP device `device`, allocates the
 * KV cache and activation buffers there.  *bytes_consumed = offset of the first byte
 * after the text model (what the reference returns as the second tuple element).
 * The host image is not referenced after return.  Q8_0, Q4_0 (group size 128) and unquantised (q_type None, f32: the reference's
 * `matmul`, functional.rs:142-171) files of the Llama / Gemma-2 / Phi families; f32 files on one GPU only.  Geometry limits (all files the
 * reference's exporter writes for its model families meet them): dim, n_heads * head_size and hidden_dim multiples of 128 - also for f32
 * files, where the reference itself only needs multiples of 8 -, head_size 64 / 96 / 128 / 256, group_size 128. */
int lmrs_create(const uint8_t* file, size_t len, int device, lmrs_ctx** out, size_t* bytes_consumed);

/* Row-sharded variant (no reference counterpart - the reference is one process on one host; replaces the same
 * Transformer::new, transformer.rs:134): this process is shard `rank` of `world`
 * (one process per GPU).  `nccl_unique_id` points at the 128-byte ncclUniqueId created
 * by rank 0 and distributed by the host (e.g. torch.distributed broadcast); it may be
 * NULL when world == 1.  NOTE: with world > 1 a NULL id does NOT fail - it selects the peer-to-peer transport: the context is created
 * unconnected and every step fails with "peers not connected" until lmrs_p2p_connect has run (lmrs_p2p_handle / lmrs_p2p_connect below;
 * at most 8 shards: the GPUs of one node).  Results are bit-identical to world == 1. */
int lmrs_create_sharded(const uint8_t* file, size_t len, int device, int rank, int world,
                        const void* nccl_unique_id, lmrs_ctx** out, size_t* bytes_consumed);

/* Writes the 128-byte ncclUniqueId for lmrs_create_sharded (call on rank 0).  No reference counterpart. */
int lmrs_comm_unique_id(void* out128);

/* Peer-to-peer transport (no reference counterpart): lmrs_create_sharded with world > 1 and nccl_unique_id == NULL makes a shard whose
 * exchanges are direct pushes into its peers' exchange arenas over xGMI (a store + flag kernel per exchange) instead of RCCL
 * all-gathers.  Every rank exports the 64-byte IPC handle of its arena, the launcher distributes all `world` handles in rank order
 * (any host transport), every rank connects; then the context is used like any other. */
int lmrs_p2p_handle(lmrs_ctx* ctx, void* out64);
int lmrs_p2p_connect(lmrs_ctx* ctx, const void* handles);

/* Host-only: the row ranges shard `rank` of `world` owns.  plan[0..9] = q-head first,count; kv-head first,count;
 * wo/w2 row first,count; gate/up pair first,count; classifier row first,count.  wo and w2 are replicated by default
 * (every shard: first 0, count dim - no gather after them); LMRS_SHARD_SPLIT_OUT=1 row-splits them as well.
 * Which matrices are split at all depends on the model and the world size: when the gate / up / down bytes a shard would stop reading
 * (3 * dim * hidden_dim * (1 - 1/world), quantised) are under ~57 MB per layer - two latency-bound exchanges per layer cost more than
 * that streams - the plan is "cls": heads, rows and pairs are all of them on every shard (the layers run whole, no exchange inside
 * them) and only the classifier rows are split: one exchange of argmax partials per token.  LMRS_SHARD_PLAN=tp|cls overrides.  (The
 * 1B / 2B models: cls at every world size; 3B / 3.8B: cls up to 4 GPUs; 8B and larger: tp.)  lmrs_create_sharded follows this plan. */
int lmrs_shard_plan(const lmrs_args* args, int rank, int world, int* plan10);
/* 1: the sharded step is one captured hipGraph (RCCL inside); 0: enqueued call by call; -1: not an RCCL shard.  No reference counterpart. */
int lmrs_shard_uses_graph(const lmrs_ctx* ctx);
/* Ranks of the context's RCCL communicator as RCCL itself counts them (ncclCommCount); 0: the context has no communicator (one GPU, or
 * the peer-to-peer transport); -1: error.  Measurement aid: lets a benchmark record that the all-gathers really spanned N ranks. */
int lmrs_comm_ranks(const lmrs_ctx* ctx);

/* Verification aid (no reference counterpart): `world` row shards of one model as `world` contexts on ONE device,
 * exchanged by device-to-device copies instead of RCCL, so the sharding can be checked bit for bit on a 1-GPU box. */
int lmrs_group_create(const uint8_t* file, size_t len, int device, int world, lmrs_ctx** shards, size_t* bytes_consumed);
/* One decode step over such a group (Transformer::forward, transformer.rs:316-384, on the sharded layout).  *logits (optional) = the assembled logits (pinned, owned by shards[0]);
 * *next (optional) = the greedy token. */
int lmrs_group_forward(lmrs_ctx** shards, int world, uint32_t token, uint32_t pos, float** logits, uint32_t* next);

/* Drop for Transformer (src/transformer.rs:688-712). */
void lmrs_destroy(lmrs_ctx* ctx);

/* `pub args` (src/transformer.rs:128). Pointer is valid for the life of ctx. */
const lmrs_args* lmrs_get_args(const lmrs_ctx* ctx);

/* ---- Transformer::forward  (src/transformer.rs:316-384) ---------------------------
 * One decode step.  *logits points at ctx-owned pinned host memory holding
 * vocab_size floats, valid (and mutable: the reference sampler scales them in place,
 * src/sampler.rs:115-117) until the next call on this ctx. */
int lmrs_forward(lmrs_ctx* ctx, uint32_t token, uint32_t pos, float** logits);

/* Same step followed by Sampler::sample_argmax (src/sampler.rs:29-41: first index of the
 * maximum) on the device; no logits leave HBM. */
int lmrs_forward_argmax(lmrs_ctx* ctx, uint32_t token, uint32_t pos, uint32_t* next);

/* Same step (Transformer::forward, src/transformer.rs:316-384) followed by the selection of the k first candidates on the device, in the order
 * lmrs_score_tokens_topk documents (rank 0 = lmrs_forward_argmax's token): idx[j] = the rank-j index, logits_k[j] = its raw f32 logit (not a
 * log-probability: a sampler applies its own temperature first).  2k words cross to the host instead of vocab_size floats; the context is left
 * as lmrs_forward leaves it.  1 <= k <= 256, k <= vocab_size.  One-GPU contexts only (extension, no reference counterpart). */
int lmrs_forward_topk(lmrs_ctx* ctx, uint32_t token, uint32_t pos, uint32_t k, uint32_t* idx /* k */, float* logits_k /* k */);

/* ---- Transformer::get_embeddings  (src/transformer.rs:659-669) -------------------- */
int lmrs_get_embeddings(const lmrs_ctx* ctx, const uint32_t* tokens, size_t n, float* out /* n*dim */);

/* ---- Transformer::fill_kv_cache  (src/transformer.rs:672-684) ---------------------
 * Runs all layers over `n` embeddings (n*dim floats, updated in place exactly as the
 * reference mutates its argument) at positions curr_pos..curr_pos+n-1; no logits.
 * *new_pos = curr_pos + n.  The supported model shapes (Q8_0 / Q4_0; Llama / Phi heads, Gemma-2) on
 * one GPU and on row-split shards run forward_layer over the whole batch (int8 matrix-core GEMMs,
 * transformer.rs:388-657 with sl = n; row shards: two all-gathers of quantised token-batch blocks
 * per layer, four when wo / w2 are split too); other shapes (f32 files, other geometries) go token
 * by token through the decode kernels.  Same values either way.
 * One documented deviation from the reference: n > 1 on a Q4_0 file (INTEGRATION.md
 * "Deviations": the reference multiplies token j with token 2j's nibbles; this computes the
 * token-by-token result). */
int lmrs_fill_kv_cache(lmrs_ctx* ctx, float* embeddings, uint32_t n, uint32_t curr_pos, uint32_t* new_pos);

/* ---- the generation loop of src/bin/chat.rs:188-222 on token IDs, greedy ------------
 * Feeds prompt[0..n_prompt) starting at position start_pos (sampler output ignored while
 * the prompt lasts, as chat.rs does: all but the last prompt token go through the batched
 * pass where lmrs_tokens_path(n_prompt - 1) says so, else token by token - same values),
 * then n_new-1 further steps feeding back the argmax.  out_tokens[i] (i < n_new) = i-th generated token, i.e. the
 * argmax after step n_prompt-1+i.  Runs device-resident: one host sync at the end.
 * *seconds (optional) = wall time of the whole call's device work (HIP events). */
int lmrs_generate_greedy(lmrs_ctx* ctx, const uint32_t* prompt, size_t n_prompt, uint32_t n_new,
                         uint32_t start_pos, uint32_t* out_tokens, double* seconds);

/* ---- scoring a token sequence (extensions, no reference counterpart) -------------------
 * Both are equivalent to calling Transformer::forward (src/transformer.rs:316-384) once per token: tokens[t] at position
 * start_pos + t for t = 0 .. n-1, in order.  K/V rows start_pos .. start_pos+n-1 are left as those calls leave them.
 * Where the shape allows (Q8_0 / Q4_0 Llama, Phi and Gemma-2 files the batched fill_kv_cache takes, classifier rows a multiple
 * of 16, n > 1) the layers and the classifier run over the whole batch on the int8 matrix cores - on Gemma-2 with forward's
 * semantics, not fill_kv_cache's: embedding rows scaled by sqrt(dim), the 4096-key window tested per position, the first `dim`
 * logits soft-capped; f32 files and other shapes run the decode step token by token.  Same values either way.  One-GPU contexts only: contexts of
 * lmrs_create_sharded / lmrs_group_create are refused.  Errors (NULL arguments, n == 0, start_pos + n > seq_len, a token
 * >= vocab_size, a sharded context) are reported before any device work and leave the context usable.
 *
 * lmrs_forward_tokens: logits[t*vocab .. (t+1)*vocab) = bit for bit what lmrs_forward(tokens[t], start_pos + t) returns after
 *   the calls for 0..t-1, for every t < n (the unwritten vocab % 4 tail of a Q8_0 / f32 classifier included, as 0.0). */
int lmrs_forward_tokens(lmrs_ctx* ctx, const uint32_t* tokens, size_t n, uint32_t start_pos, float* logits /* n*vocab */);
/* lmrs_score_tokens: the same pass with the logits kept on the device.
 *   argmax[t] (n entries, may be NULL): Sampler::sample_argmax of position t (sampler.rs:29-41: first index of the maximum, the
 *     unwritten vocab % 4 tail counting as 0.0), as lmrs_forward_argmax.
 *   logprobs[t] (n-1 entries, may be NULL): log softmax(logits_t)[tokens[t+1]], defined as follows.  m = the f32 maximum of the
 *     vocab_size logits, widened to double; lp = (double)l[y] - m - log(sum_i exp((double)l_i - m)), the sum in double over all
 *     vocab_size logits (zero tail included); logprobs[t] = lp rounded once to float.
 *   *sum_logprob (may be NULL): the sum of the n-1 unrounded lp, in double, in position order (0.0 for n = 1). */
int lmrs_score_tokens(lmrs_ctx* ctx, const uint32_t* tokens, size_t n, uint32_t start_pos,
                      float* logprobs, uint32_t* argmax, double* sum_logprob);
/* lmrs_score_tokens_topk: lmrs_score_tokens - the same pass, K/V rows, error rules and refusal of sharded contexts, and logprobs, argmax and
 *   *sum_logprob bit for bit its results - with the k first next-token candidates of every position, 1 <= k <= 256, k <= vocab_size (else an
 *   error before any device work).  The candidate order: all vocab_size logits take part (the unwritten tail as 0.0); the larger value first,
 *   -0.0 == +0.0; equal values by ascending index (sample_argmax's "first index of the maximum", extended); a NaN after every number, NaNs by
 *   ascending index - but a NaN at index 0 takes rank 0, as sampler.rs:29-41 never displaces it: rank 0 is argmax[t] in every case.
 *   topk_idx[t*k + j] (n*k entries): the rank-j index of position t.
 *   topk_logprob[t*k + j] (n*k entries): (double)l[idx] - m - log(sum) rounded once to float, with the m and the sum of logprobs[t]: where
 *     tokens[t+1] is among the k its entry equals logprobs[t] bit for bit.
 *   target_rank[t] (n-1 entries, may be NULL): the number of candidates that precede tokens[t+1] in that order (0: it is the argmax), exact for
 *     any rank - it is counted over the whole row, not capped at k. */
int lmrs_score_tokens_topk(lmrs_ctx* ctx, const uint32_t* tokens, size_t n, uint32_t start_pos, uint32_t k,
                           float* logprobs, uint32_t* argmax, double* sum_logprob,
                           uint32_t* topk_idx /* n*k */, float* topk_logprob /* n*k */, uint32_t* target_rank /* n-1, may be NULL */);

/* ---- a prompt from token ids (extension, no reference counterpart) ---------------------
 * Equivalent to calling Transformer::forward (src/transformer.rs:316-384) for tokens[t] at position start_pos + t, t = 0 .. n-1,
 * and discarding every logits vector: K/V rows start_pos .. start_pos+n-1 are left bit for bit as those calls leave them.
 * The logits buffer of lmrs_forward is unspecified afterwards.  *new_pos (may be NULL) = start_pos + n.
 * The token ids go to the device and the layers run over the run on the int8 matrix cores, 512 tokens at a time, where
 * lmrs_tokens_path says so (neither the final norm nor the classifier runs); else one decode step per token with the classifier's
 * result ignored.  Same rows either way.  Unlike lmrs_get_embeddings + lmrs_fill_kv_cache this has forward's semantics on Gemma-2
 * (rows scaled by sqrt(dim), the window per position) and moves no activations through host memory.  Row-sharded contexts with a
 * transport are accepted (every rank makes the same call).  Errors (NULL arguments, n == 0, start_pos + n > seq_len, a token >=
 * vocab_size) are reported before any device work and leave the context usable. */
int lmrs_prefill_tokens(lmrs_ctx* ctx, const uint32_t* tokens, size_t n, uint32_t start_pos, uint32_t* new_pos);
/* Which path lmrs_prefill_tokens (and the prompt of lmrs_generate_greedy, for a prompt of n + 1 tokens) takes for a run of n tokens on
 * this context: *batched = 1 the matrix-core pass, 0 token by token.  (lmrs_forward_tokens / lmrs_score_tokens keep their own rule:
 * n > 1, a batched-eligible file, classifier rows a multiple of 16.) */
int lmrs_tokens_path(const lmrs_ctx* ctx, size_t n, int* batched);

/* ---- short runs in one weight pass: verifying drafted tokens (extensions, no reference counterpart) -------------------
 * lmrs_verify_tokens replaces n calls of Transformer::forward (src/transformer.rs:316-384) + Sampler::sample_argmax (sampler.rs:29-41):
 * tokens[0] at start_pos is the last confirmed token, tokens[1..n) are drafts.
 *   argmax[t] (n entries) = lmrs_forward_argmax(tokens[t], start_pos + t) after the calls for 0..t-1.
 *   *n_accept = the number of leading drafts with tokens[t+1] == argmax[t]  (0 .. n-1).
 * K/V rows start_pos .. start_pos+n-1 are left as those calls leave them; rows past start_pos + *n_accept belong to rejected drafts
 * and are rewritten by whatever runs at those positions next.  2 <= n <= 16.
 * After a partial acceptance the next pass starts at start_pos + *n_accept + 1 with argmax[*n_accept] as its tokens[0] (argmax[0 .. *n_accept]
 * are the *n_accept + 1 tokens the call has produced).
 * Where lmrs_score_tokens would run its batched pass the run goes through that chain with every GEMM - the layers' and the classifier - in the
 * skinny weight-streaming form: the weights cross HBM once for the n tokens.  f32 files, other geometries, LMRS_NO_BATCHED_PREFILL=1 and classifier
 * rows that are no multiple of 16 run the decode step per token: same values.  One-GPU contexts only.  Errors (NULL arguments, n outside 2 .. 16,
 * start_pos + n > seq_len, a token >= vocab_size, a sharded context) are reported before any device work and leave the context usable. */
int lmrs_verify_tokens(lmrs_ctx* ctx, const uint32_t* tokens, size_t n, uint32_t start_pos, uint32_t* argmax, uint32_t* n_accept);

/* Host only, no device: prompt-lookup drafting (no reference counterpart).  The longest suffix of hist[0..n_hist) of length <= ngram_max (>= 1)
 * that also occurs earlier in hist (an occurrence that starts before the suffix does; it may overlap it); the tokens that followed its LATEST
 * earlier occurrence, at most max_draft of them and never past the end of hist -> draft, *n_draft (0: no match, also for n_hist < 2). */
int lmrs_draft_lookup(const uint32_t* hist, size_t n_hist, uint32_t ngram_max, uint32_t max_draft, uint32_t* draft, uint32_t* n_draft);

/* lmrs_generate_greedy's contract and out_tokens, bit for bit (the loop of src/bin/chat.rs:188-222 at temperature 0), produced by draft
 * (lmrs_draft_lookup over prompt + output so far) and verify (lmrs_verify_tokens' pass); a position without a draft is one ordinary decode
 * step (lmrs_forward_argmax).  max_draft 1..15, ngram_max >= 1.  The loop synchronises with the host once per pass or step.
 * stats4 (may be NULL; four counts, each at most n_new): [0] verify passes, [1] drafted tokens, [2] accepted tokens, [3] plain decode steps; a pass yields its accepted drafts
 * and one more token, a plain step one token, and the last pass is never drafted past n_new:  [0] + [2] + [3] == n_new,  [2] <= [1].
 * *seconds (optional) = host wall time of the whole call.  One-GPU contexts only; errors as lmrs_generate_greedy's, before any device work. */
int lmrs_generate_speculative(lmrs_ctx* ctx, const uint32_t* prompt, size_t n_prompt, uint32_t n_new, uint32_t start_pos,
                              uint32_t max_draft, uint32_t ngram_max, uint32_t* out_tokens, uint32_t* stats4, double* seconds);

/* ---- multi-sequence decode: up to 16 sequences a step over one copy of the weights (extensions, no reference counterpart) -------------------
 * A batch is n_slots K/V caches beside the context's own; a step (lmrs_batch_forward) is ONE weight pass - the skinny form of lmrs_verify_tokens'
 * pass - whose rows are tokens of DIFFERENT sequences, each at its own position over its own slot.  Every output is bit for bit what the same tokens
 * give through lmrs_forward / lmrs_forward_argmax on a context that holds only that sequence (Gemma-2: rows scaled by sqrt(dim), the window per row,
 * both soft caps).  The context's own cache is a 17th, private sequence: no batch call changes anything a call on ctx can observe, and batch and
 * context calls may interleave freely.
 * Errors (NULL arguments, n outside 1 .. 16, a slot >= n_slots, a slot twice in one call, a token >= vocab_size, pos (+ n_new - 1) >= seq_len,
 * fork with n_pos > seq_len or src == dst) are reported before any device work and leave ctx and batch usable. */
#define LMRS_BATCH_CTX 0xFFFFFFFFu   /* lmrs_batch_fork's src_slot: the context's own cache */
typedef struct lmrs_batch lmrs_batch;

/* n_slots KV caches (1 .. 16) beside ctx's own, same layout and seq_len, on ctx's device; ctx's weights,
 * stream and scratch are shared (ctx and its batches are ONE not-thread-safe object; destroy batches first).
 * Refused, each with its own message: sharded and group contexts; contexts without the batched pass for short runs (f32 files, other
 * geometries, classifier rows that are no multiple of 16, LMRS_NO_BATCHED_PREFILL=1) - there is no token-by-token form.  Allocation is
 * all or nothing; the message gives the bytes wanted (n_slots * 2 * n_layers * seq_len * kv_dim * 4). */
int  lmrs_batch_create(lmrs_ctx* ctx, uint32_t n_slots, lmrs_batch** out);
void lmrs_batch_destroy(lmrs_batch* b);
/* lmrs_batch_create with up to 64 slots: a WIDE batch.  Same refusals (each message opens with this call's name), same allocation rule (all or
 * nothing, the message gives the bytes).  On a wide batch every batch call below works as documented with 64 where it says 16: lmrs_batch_forward
 * and lmrs_batch_generate_greedy take n up to 64, lmrs_batch_forward_runs up to 64 runs (still at most 512 rows), slots go up to 63; a pass of
 * 17 .. 64 rows is still ONE weight pass (up to 47 rows gemm_stream_kernel: the skinny kernel's weight stream against 2 .. 3 token tiles; from 48
 * on the ring kernels of the batched pass) and every output is bit for bit the single-sequence value.  Calls with 16 rows or fewer take the same path as on a batch of lmrs_batch_create.
 * lmrs_batch_forward_sample keeps 16 rows a call on any batch. */
int  lmrs_batch_create_wide(lmrs_ctx* ctx, uint32_t n_slots /* 1 .. 64 */, lmrs_batch** out);
/* 16 for lmrs_batch_create's batches, 64 for wide ones: the most rows (lmrs_batch_forward, _generate_greedy) and runs (_forward_runs) a call takes. */
int  lmrs_batch_width(const lmrs_batch* b, uint32_t* width);
/* ---- paged K/V (extensions, no reference counterpart): a WIDE batch (width 64) whose slots draw pages of page_len positions from ONE pool of n_pages
 * pages instead of holding a whole cache each.  Same refusals as lmrs_batch_create (each message opens with this call's name); also refused: a
 * page_len other than 64, 128, 256, 512, 1024, and n_pages == 0.  The allocation is (n_pages + 1) * 2 * n_layers * page_len * kv_dim * 4 bytes, all or
 * nothing, the message gives the bytes.  The extra page is page 0, the ZERO PAGE: cleared at create, never written; every page-table entry of every
 * slot starts there, so a position nobody wrote reads as zero, exactly as in a fresh contiguous slot.
 * Every batch call works on a paged batch as documented for a wide batch, and - for any sequence of calls without lmrs_batch_release - returns what a
 * lmrs_batch_create_wide batch returns, bit for bit: tokens, logits, top-k, sampled tokens, sampler state, lmrs_batch_debug_kv rows.  Paging changes
 * addresses only, never the order of a floating-point operation.
 * Page accounting, decided on the host and finished before any device work of a call.  A call that writes positions [p0, p1) of a slot (a prefill, a
 * run, a decode row, all n_new steps of lmrs_batch_generate_greedy up front) takes, per page the range touches: a free page, cleared in stream order,
 * where the entry is 0; a free page with the whole old page copied into it where the entry has more than one holder (copy on write; the old
 * reference is dropped); nothing where the slot holds the page alone.  A call that needs more free pages than there are fails with a message of its
 * own - the call's name, pages wanted, pages free - and has changed nothing: batch, context and samplers stay usable.
 * lmrs_batch_fork(src, dst, n_pos): dst's entries of the pages wholly inside [0, n_pos) become references to src's pages (dst's former pages there are
 * dropped); the rows of the partial last page are copied into a page dst holds alone; dst's later entries stay.  At most one page copy and a table
 * edit.  From LMRS_BATCH_CTX (a contiguous cache) the rows are copied into dst's own pages.
 * Prompts: lmrs_batch_prefill and lmrs_batch_prefill_embeddings run chunks of at most 512 rows on a paged batch; a chunk of 112 rows or more takes block
 * attention over the page table (64-query blocks, one table lookup per 64-key chunk or tile) under the contiguous rule - head sizes 64 / 96 / 128, Gemma's
 * 256, at most 1 GiB of score slabs -, a shorter one the table pass, one workgroup per (head, row), which measures faster there; the values are the same
 * bits either way (lmrs_batch_prefill_form tells how a call would run).  512 tokens of Llama-3.2-1B Q8_0: 2.73 ms against 2.59 ms on a wide batch (1.05x;
 * the table pass took 5.91 ms), Gemma-2-2B Q4_0 7.85 against 7.57 ms (1.04x; 12.44) (profiles/batch_paged_prefill_*.txt).  A decode pass of 64 rows costs +2.9 % at 100 positions and +4.7 % at 1000 on Llama-3.2-1B Q8_0 and is
 * 0.7 % / 5.7 % faster on Gemma-2-2B Q4_0 (profiles/batch_paged_llama1b.txt, profiles/batch_paged_gemma2b_q4.txt). */
int lmrs_batch_create_paged(lmrs_ctx* ctx, uint32_t n_slots /* 1 .. 64 */, uint32_t page_len /* 64, 128, 256, 512 or 1024 */,
                            uint32_t n_pages /* >= 1 */, lmrs_batch** out);
/* the pool: its page length, its pages (the zero page not counted) and how many of them nobody holds.  Refused on a batch that is not paged. */
int lmrs_batch_pages(const lmrs_batch* b, uint32_t* page_len, uint32_t* n_pages, uint32_t* n_free);
/* the pages a slot holds, and how many of them have more than one holder.  Refused on a batch that is not paged, and for a slot >= n_slots. */
int lmrs_batch_slot_pages(const lmrs_batch* b, uint32_t slot, uint32_t* n_held, uint32_t* n_shared);
/* keep positions [0, n_pos) of a slot (0 empties it): the slot's references to the pages at index ceil(n_pos / page_len) and above are dropped, those
 * entries return to the zero page, and a page nobody holds is free.  Refused, each with its own message: a batch that is not paged, a slot >=
 * n_slots, n_pos > seq_len. */
int lmrs_batch_release(lmrs_batch* b, uint32_t slot, uint32_t n_pos);
/* (extension, no reference counterpart)
 * How lmrs_batch_prefill / lmrs_batch_prefill_embeddings would run n rows at start_pos on this batch:
 * *n_chunks = passes of at most 512 rows, *n_block = how many of them take block attention (64-query blocks);
 * the others take one workgroup per (head, row).  Host arithmetic only; any batch, paged or not.  Refused: NULL arguments, start_pos + n > seq_len. */
int lmrs_batch_prefill_form(const lmrs_batch* b, size_t n, uint32_t start_pos, uint32_t* n_chunks, uint32_t* n_block);
/* (extension, no reference counterpart)
 * Test / A-B aid in lmrs_debug_inject's manner (an explicit call; nothing is read from the environment): force != 0 -
 * every prompt chunk of this PAGED batch takes the table pass from now on (the routing before block attention read the page table); 0 - the
 * library's rule.  Refused on a batch that is not paged. */
int lmrs_batch_debug_prefill_table(lmrs_batch* b, int force);

/* == lmrs_prefill_tokens, into slot's cache: rows start_pos .. start_pos+n-1 as n forward calls leave them */
int lmrs_batch_prefill(lmrs_batch* b, uint32_t slot, const uint32_t* tokens, size_t n, uint32_t start_pos);

/* rows [0, n_pos) of every layer, K and V: src -> dst (LMRS_BATCH_CTX as src = ctx's own cache): a shared
 * system prompt or best-of-n prefilled once */
int lmrs_batch_fork(lmrs_batch* b, uint32_t src_slot, uint32_t dst_slot, uint32_t n_pos);

/* ONE weight pass for n rows (1 .. 16), row i = Transformer::forward(tokens[i], pos[i]) (src/transformer.rs:316-384) on slot[i]'s cache +
 * Sampler::sample_argmax (sampler.rs:29-41).  Slots distinct within a call, any order, any subset.
 * argmax[i] (n); logits (may be NULL): n*vocab floats as lmrs_forward_tokens writes a row. */
int lmrs_batch_forward(lmrs_batch* b, uint32_t n, const uint32_t* slot, const uint32_t* tokens,
                       const uint32_t* pos, uint32_t* argmax, float* logits);

/* n_new greedy steps for n rows, device-resident, one host sync at the end.
 * out_tokens[i*n_new + j] = argmax after feeding row i's j-th token (the first is tokens[i] at pos[i]):
 * per row lmrs_generate_greedy's out_tokens for a one-token prompt on that slot.  *seconds optional (HIP events). */
int lmrs_batch_generate_greedy(lmrs_batch* b, uint32_t n, const uint32_t* slot, const uint32_t* tokens,
                               const uint32_t* pos, uint32_t n_new, uint32_t* out_tokens, double* seconds);

/* ONE weight pass over n_runs runs (1 .. 16).  Run i = tokens[t_i .. t_i + run_len[i]) (t_i = sum of the earlier run_len) at positions
 * start_pos[i] .. start_pos[i] + run_len[i] - 1 of slot[i]: per row Transformer::forward (src/transformer.rs:316-384) on a context that
 * holds only that sequence, in position order - a prompt (chunk) to admit, a draft to verify, or one decode row, mixed freely; at most 512
 * rows in all, a slot in at most one run.  Outputs for the LAST n_out[i] rows of run i (0: K/V rows only), packed in run order, ascending
 * position within a run; O = sum of n_out (O == 0: neither the final norm nor the classifier runs).
 *   argmax (O; may be NULL when O == 0): Sampler::sample_argmax (sampler.rs:29-41) of every output row;
 *   logits (may be NULL): O * vocab floats as lmrs_forward_tokens writes a row;
 *   k > 0: topk_idx / topk_logprob (O * k each), order and log-probability exactly as lmrs_score_tokens_topk defines them; k <= 256, k <= vocab.
 * K/V rows are left as the per-token calls leave them; rows of rejected drafts are stale and rewritten by whatever runs at those positions
 * next, as with lmrs_verify_tokens.  Errors, each with a message of its own and before any device work: a NULL array, n_runs outside 1 .. 16, a
 * run_len of 0, more than 512 rows, a slot >= n_slots or in two runs, n_out > run_len, start_pos + run_len > seq_len, a token >= vocab_size, k
 * out of range or without its two arrays, O > 0 without argmax. */
int lmrs_batch_forward_runs(lmrs_batch* b, uint32_t n_runs, const uint32_t* slot, const uint32_t* start_pos, const uint32_t* run_len,
                            const uint32_t* n_out, const uint32_t* tokens, uint32_t* argmax, float* logits,
                            uint32_t k, uint32_t* topk_idx, float* topk_logprob);

/* verification aid, as lmrs_debug_kv */
int lmrs_batch_debug_kv(lmrs_batch* b, uint32_t slot, int which, uint32_t layer, uint32_t pos, float* out);

const char* lmrs_last_error(void);

/* ---- L2 free functions, for unit parity (host pointers in and out) ------------------
 * Each runs the SAME device kernel the decode path uses, on device `device`.          */
/* functional.rs:173-214.  x: sl rows of n int8 + sl*n/gs scales; w: o*n int8 + o*n/gs scales. */
int lmrs_op_matmul_q8(int device, float* xout, const int8_t* xq, const float* xs,
                      const int8_t* wq, const float* ws, size_t n, size_t o, size_t gs, size_t sl);
/* functional.rs:216-250 (decode form, sl = 1).  xq: n/2 bytes, wq: o*n/2 bytes. */
int lmrs_op_matmul_q4(int device, float* xout, const uint8_t* xq, const float* xs,
                      const uint8_t* wq, const float* ws, size_t n, size_t o, size_t gs);
/* quantization.rs:44-67 */
int lmrs_op_quantize(int device, int8_t* q, float* s, const float* x, size_t n, size_t gs);
/* quantization.rs:69-95 */
int lmrs_op_quantize_q4(int device, uint8_t* q, float* s, const float* x, size_t n, size_t gs);
/* functional.rs:48-78 */
int lmrs_op_rmsnorm(int device, float* o, const float* x, const float* weight, size_t size, float eps, int add_unit_offset);
/* functional.rs:122-140 (in place) */
int lmrs_op_softmax(int device, float* x, size_t n);
/* The decode step's classifier launch + final argmax on caller-supplied rows: final rmsnorm + quantize + matmul_q8 (transformer.rs:341-381)
 * and Sampler::sample_argmax (sampler.rs:29-41: starts at index 0, moves on a strict `>`: first index of the maximum; a NaN at index 0
 * is never displaced, NaNs elsewhere never win).  logits (optional): the o logits. */
int lmrs_op_classifier_argmax(int device, const float* x, const float* rms_w, const int8_t* wq, const float* ws, size_t n, size_t o,
                              float eps, uint32_t* token, float* logits);
/* f32::exp as used by softmax (functional.rs:133) and SiLU (transformer.rs:617): the device's bit-exact restatement of glibc expf. */
int lmrs_op_expf(int device, float* y, const float* x, size_t n);
/* y = (float)tanh(c * (double)x): f64::tanh as the reference calls it for Gemma's soft-caps (transformer.rs:520-522, 377-379; c = 1) and
 * the tanh-GELU (transformer.rs:614; c = 0.7978845608028654) - the device's f64 tanh, for comparison with the host libm (oracle/tanh_check.c). */
int lmrs_op_tanh_cast(int device, float* y, const float* x, size_t n, double c);
/* Sampler::sample (sampler.rs:109-129) for temperature != 0 and sample_mult on caller-supplied logits through lmrs_forward_sample's route (scaling,
 * maximum and exponentials on the device, the two sequential chains on the host): they are scaled and softmax-ed IN PLACE (as the reference does
 * to the slice) and *token = the draw for the random number rnd.  Unit parity for lmrs_forward_sample. */
int lmrs_op_sample_mult(int device, float* logits, size_t n, float temperature, float rnd, uint32_t* token);
/* The kernels of lmrs_batch_forward_sample on caller-supplied rows: Sampler::sample (sampler.rs:109-129) for n_rows (1 .. 16) rows of n logits (any
 * n >= 1), row r with temperature[r], top_p[r] and the random number rnd[r], everything on the device.  rows: scaled and softmax-ed IN PLACE (rows of
 * temperature 0 are not touched).  sample_mult rows (top_p <= 0 or >= 1): token[r] = the draw (sampler.rs:43-55).  top-p rows: n0[r] = the candidates
 * with prob >= (1 - top_p) / (n - 1) and, if pairs != NULL, pairs[r * n .. r * n + n0[r]) = {f32 prob, u32 index} in ascending index order - what
 * sampler.rs:74-80 leaves in probindex[0 .. n0) and what lmrs_sampler_topp_pairs takes.  token / n0 of the other rows: 0.  Everything else is refused
 * before the device is touched. */
int lmrs_op_sample_rows(int device, float* rows, size_t n_rows, size_t n, const float* temperature, const float* top_p, const float* rnd,
                        uint32_t* token, uint32_t* n0, void* pairs);
/* Measurement: the six launches behind lmrs_op_sample_rows (scale + maxima, exponentials, the sum chain, the division, the cdf chain, the ordered
 * candidates) on n_rows rows of n logits whose chains walk all n terms: us6[k] = device microseconds of launch k summed over iters runs (HIP events
 * on the dispatches, one warm-up run before them); *clock_mhz (optional) = the device's nominal shader clock.  tools/sample_rate.py turns launches 2
 * and 4 into cycles per term. */
int lmrs_bench_sample_rows(int device, size_t n_rows, size_t n, int iters, double* us6, double* clock_mhz);
/* Measurement: the launches behind lmrs_op_topp_rows on n_rows (1 .. 64) rows of n0 (1 .. n) candidates each, probabilities scattered, over vectors of n
 * (2 .. 2^24) entries that carry the runs before: *us = device microseconds of all launches of one run (HIP events on the dispatches, summed), the
 * mean of iters runs after one warm-up; *launches (optional): how many launches a run has - vocab_size alone decides. */
int lmrs_bench_topp_rows(int device, size_t n_rows, size_t n, size_t n0, int iters, double* us, int* launches);
/* The selection kernels of lmrs_score_tokens_topk / lmrs_forward_topk on one caller-supplied row of n logits of which the first `written` exist
 * (the rest count as 0.0 and are never read): idx[j], val[j] = the rank-j index and its raw value, j < k.  Unit parity for the ordering rule (NaNs,
 * signed zeros, equal values, k = n); extension, no reference counterpart.  k = 0, k > 256 and k > n are refused before the device is touched. */
int lmrs_op_topk(int device, const float* logits, size_t n, size_t written, uint32_t k, uint32_t* idx, float* val);

/* ---- measurement hooks (bench.py) ---------------------------------------------------
 * Runs, `iters` times, the dequant-GEMV launches of ONE decode step in step order (per layer: qkv, wo,
 * w1w3, w2; then the classifier) so the weight stream is the real one, each launch bracketed by HIP events
 * on the context's stream.  Index k of the outputs: 0 qkv, 1 wo, 2 w1w3, 3 w2, 4 classifier;
 * us5[k] = summed duration (microseconds), bytes5[k] = summed algorithmic bytes (int8 + f32 scales),
 * count5[k] = launches.  Activations hold garbage afterwards; weights and older KV rows are untouched. */
int lmrs_bench_gemv(lmrs_ctx* ctx, int iters, double* us5, double* bytes5, int* count5);
/* The real decode step at position `pos` (then pos+1, ...) replayed eagerly `iters` times from the context's live state with HIP events on
 * every dispatch: per-kernel durations as they occur INSIDE the step.  kind k: 0 qkv, 1 attention, 2 wo, 3 w1w3, 4 w2, 5 classifier,
 * 6 argmax + next embedding row, 7 glue launches of the sharded / unfused forms, 8 peer-to-peer exchanges (time waiting for the peers
 * included); us9[k] = summed duration, bytes9[k] = summed algorithmic bytes, count9[k] = launches.  On a row-sharded context every
 * rank calls it together.  Measurement aid, no reference counterpart; the decode state advances by `iters` + 1 valid greedy steps. */
int lmrs_bench_step(lmrs_ctx* ctx, uint32_t pos, int iters, double* us9, double* bytes9, int* count9);
/* Debug timeline (LMRS_DEBUG_TIMELINE=1 in the environment at lmrs_create): 8 wall-clock stamps (100 MHz) per
 * kernel of the last decode step, in launch order: [0..3] first workgroup, [4..7] last workgroup:
 * start, prologue done, first rows done, end. */
int lmrs_debug_timeline(lmrs_ctx* ctx, unsigned long long* out, int max_nodes, int* n_nodes);
/* Verification aid (no reference counterpart; the reference's key_cache / value_cache are private, transformer.rs:302-303): one row of
 * the KV cache as the reference lays it out (which: 0 key, 1 value; kv_dim floats of `layer` at `pos`). */
int lmrs_debug_kv(lmrs_ctx* ctx, int which, uint32_t layer, uint32_t pos, float* out);
/* Device time (ms, HIP events) the last BATCHED lmrs_fill_kv_cache of this context spent between the upload of its embeddings and the
 * download of the residual stream: forward_layer(sl = n) itself.  Measurement aid (bench.py's `prefill` object), no reference counterpart. */
int lmrs_last_fill_ms(const lmrs_ctx* ctx, double* ms);
/* Fault injection for the tests of the multi-GPU paths (no reference counterpart; explicit calls, nothing is read from the environment):
 *   what = 0: the next lmrs_p2p_connect of this context fails ("injected failure"), so that a launcher's "every rank falls back
 *             together" logic can be exercised;
 *   what = 1: a row-sharded context enqueues its steps eagerly from now on and spins `b` microseconds on the device right after the
 *             exchange that follows segment `a` of every step (4 * n_layers = the argmax partials) - a peer that runs ahead then pushes
 *             its next block while this shard has not consumed the current one. */
int lmrs_debug_inject(lmrs_ctx* ctx, int what, int a, int b);
/* Number of kernel launches per decode step and the sum of algorithmic bytes per step at `pos` (the byte model of SURVEY.md §8d;
 * measurement aid, no reference counterpart). */
int lmrs_step_info(const lmrs_ctx* ctx, uint32_t pos, int* n_launches, double* algo_bytes);
/* The output tile (weight rows x tokens per workgroup, waves per workgroup) the batched matmul_q8 / matmul_q4 (functional.rs:173-250 with
 * sl = n_tok) runs a launch of `o` rows over K = `n` with: the cost model of DESIGN.md section 4.1, host arithmetic only (no device is
 * touched).  0 x 0: fewer than 48 tokens - the direct kernels.  Inspection aid, no reference counterpart. */
int lmrs_debug_gemm_tile(uint32_t n, uint32_t o, uint32_t n_tok, int q4, int* tile_rows, int* tile_tokens, int* waves);
/* The batched w1 / w3 projection with the activation and the NEXT matmul's quantiser in its epilogue, as fill_kv_cache runs it from a few
 * hundred tokens on (transformer.rs:588-630 with sl = n_tok: matmul_q8, SiLU(gate) * up or GELU(gate) * up, quantize): `wq` holds o rows of n
 * int8 with gate / up rows interleaved (row 2i = w1's row i, row 2i + 1 = w3's), hq receives n_tok x o/2 int8 and hs n_tok x o/256 scales.
 * Returns -1 with a message when the shape does not take the fused epilogue (lmrs_debug_gemm_tile: fewer than 128 rows x 128 tokens per
 * tile).  Unit-parity aid, no reference counterpart. */
int lmrs_debug_w13_quant(int device, int8_t* hq, float* hs, const int8_t* xq, const float* xs, const int8_t* wq, const float* ws,
                         size_t n, size_t o, size_t n_tok, int gemma);
/* The skinny weight-streaming GEMM of lmrs_verify_tokens' pass (gemm_skinny_kernel; matmul_q8 / matmul_q4 of functional.rs:173-250 with
 * sl = n_tok, 1 <= n_tok <= 16) on caller-supplied operands: out[t*o + r], n a multiple of 256, o of 16, row-major scales.  q4 = 0: xq n_tok x n int8,
 * wq o x n int8.  q4 = 1: xq n_tok x n/2 and wq o x n/2 packed bytes as the reference packs Q4_0 (the hook de-interleaves the activations into the
 * int8 rows the batched pass keeps).  Unit-parity aid, no reference counterpart. */
int lmrs_debug_gemm_skinny(int device, float* out, const int8_t* xq, const float* xs, const uint8_t* wq, const float* ws,
                           size_t n, size_t o, size_t n_tok, int q4);
/* The same for the stream GEMM of a batch pass of 17 .. 47 rows (gemm_stream_kernel), here at any 1 <= n_tok <= 64: lmrs_debug_gemm_skinny's operands and
 * shape rules; anything else is refused with this hook's name in the message. */
int lmrs_debug_gemm_wide(int device, float* out, const int8_t* xq, const float* xs, const uint8_t* wq, const float* ws,
                         size_t n, size_t o, size_t n_tok, int q4);

/* ---- CLIP image tower of the multimodal models  (src/vision.rs) ---------------------------
 * lmrs_vision_create   <- VisionTransformer::new(data) -> (VisionTransformer, usize)   vision.rs:99-243
 *   `section` points at the vision section of an LMRS multimodal file (offset = *bytes_consumed of lmrs_create);
 *   *bytes_consumed = size of the section (the processor section follows).  CLIP ViT-L/14-336 geometry; Q8_0 (the tuned path),
 *   Q4_0 (quantize_q4 rows, matmul_q4 from packed nibbles on the matrix cores) and q_type None (the f32 `matmul`, correct, not tuned).
 * lmrs_vision_forward  <- VisionTransformer::forward(pixel_values, num_crops) -> (Vec<f32>, u32)   vision.rs:244-577
 *   pixel_values: num_crops * 3 * image_size^2 floats, normalised and cut into patches as PHI3VProcessor::process
 *   produces them; out: num_crops * 576 * dim floats (class token dropped); *new_shape = 576 * dim.
 *   Projections run as int8 matrix-core GEMMs over all tokens of all crops; the f32x8 lane structure of the
 *   reference's layernorm / matmul_rest sums (and the patch-embedding tail quirk) is reproduced: same values. */
typedef struct lmrs_vision lmrs_vision;
int lmrs_vision_create(const uint8_t* section, size_t len, int device, lmrs_vision** out, size_t* bytes_consumed);
void lmrs_vision_destroy(lmrs_vision* v);
int lmrs_vision_forward(lmrs_vision* v, const float* pixel_values, uint32_t num_crops, float* out, uint32_t* new_shape);

/* --------------------------------------------------------------------------------------------------------------------------
 * Image projector of the multimodal models (reference src/processor.rs, struct PHI3VProcessor).  Q8_0, Q4_0 and unquantised sections.
 *
 * lmrs_processor_create   <- PHI3VProcessor::new(data) -> PHI3VProcessor              processor.rs:168-232
 *     section = the bytes that follow the vision tower's section in the model file (128-byte header: hidden_dim, text_dim,
 *     q_type, group_size; glb_GN, sub_GN, the two projections, their biases).
 * lmrs_processor_forward  <- PHI3VProcessor::forward(out_patches, new_shape, patch_side, w_crop, h_crop) -> (Vec<f32>, u32)
 *                                                                                       processor.rs:234-342
 *     out_patches = lmrs_vision_forward's output (global crop first), total_floats floats; the HD transform
 *     (reshape_hd_patches_2x2merge :377-418, add_image_newline :480-484), the separators and the two-layer tanh-GELU MLP;
 *     out receives n_embeds * text_dim floats, n_embeds = (h_crop*12)*(w_crop*12+1) + 12*13 + 1.
 * lmrs_processor_destroy  <- Drop
 */
typedef struct lmrs_processor lmrs_processor;
int lmrs_processor_create(const uint8_t* section, size_t len, int device, lmrs_processor** out, size_t* bytes_consumed);
void lmrs_processor_destroy(lmrs_processor* p);
int lmrs_processor_forward(lmrs_processor* p, const float* out_patches, uint32_t total_floats, uint32_t new_shape, uint32_t patch_side,
                           uint32_t w_crop, uint32_t h_crop, float* out, uint32_t* n_embeds);
/* Host-only verification aid (works without a GPU): the rows lmrs_processor_forward feeds to the projector - the HD transform
 * reshape_hd_patches_2x2merge + add_image_newline (processor.rs:377-418, 480-484) of the sub-images, glb_GN, the same of the
 * global crop (:240-254) - for given separators.  out: n_embeds * 4096 floats. */
int lmrs_processor_hd_transform(const float* out_patches, uint32_t total_floats, uint32_t new_shape, uint32_t w_crop, uint32_t h_crop,
                                const float* glb_gn, const float* sub_gn, float* out, uint32_t* n_embeds);

/* Host-only verification aid (works without a GPU): the (cos, sin) pair lmrs_create tabulates for position `pos` and pair `j` of a
 * head (j < head_size / 2) - the RoPE frequency arithmetic of transformer.rs:446-477 (Llama-3 wavelength scaling, Phi LongRoPE short
 * factors and magnitude) for the model family / rope_theta / head_size in `args`.  Lets the tests check this host function against a
 * transcription that shares no code with it. */
int lmrs_rope_terms(const lmrs_args* args, uint32_t pos, uint32_t j, float* fcr, float* fci);

/* --------------------------------------------------------------------------------------------------------------------------
 * The callers either side of the device path, HOST code with the reference's exact results (no GPU needed):
 *
 * lmrs_tokenizer_create   <- Tokenizer::new(path)   src/tokenizer.rs:24-64   (data = the bytes of tokenizer.bin)
 * lmrs_tokenizer_encode   <- Tokenizer::encode(text, bos, eos, chat_format, model_type) -> Vec<u32>   :66-151
 *     one id per character (or its UTF-8 bytes + 3), then greedy merging of the best-scoring adjacent pair; chat_format wraps the
 *     ids in the model family's hard-coded template ids.  model_type: 0 GEMMA, 1 LLAMA, 2 PHI.  *n = ids produced (<= cap).
 * lmrs_tokenizer_decode   <- Tokenizer::decode(token) -> String   :153-163   (bytes, not NUL-terminated; "<0xHH>" -> U+00HH)
 * lmrs_tokenizer_info     <- the pub fields bos / eos (:15-16) and vocab_size
 *
 * lmrs_sampler_create     <- Sampler::new(vocab_size, temperature, top_p, seed)   src/sampler.rs:19-27
 * lmrs_sampler_sample     <- Sampler::sample(&mut logits) -> u32   :109-129: temperature 0 -> sample_argmax (:29-41); otherwise the
 *     logits are divided by the temperature and softmax-ed IN PLACE (functional.rs:122-140, one sequential sum - which is why this
 *     stays on the host: see lmrs_text.cpp) and sample_mult (:43-55) or sample_topp (:67-106) draws with random_f32(seed)
 *     (functional.rs:34-44).  The reference never advances the seed (:119) - every call of one Sampler uses the same random
 *     number - and sorts its whole candidate vector, stale entries included (:81): both reproduced. */
typedef struct lmrs_tokenizer lmrs_tokenizer;
int lmrs_tokenizer_create(const uint8_t* data, size_t len, lmrs_tokenizer** out);
void lmrs_tokenizer_destroy(lmrs_tokenizer* t);
int lmrs_tokenizer_info(const lmrs_tokenizer* t, uint32_t* vocab_size, uint32_t* bos, uint32_t* eos);
int lmrs_tokenizer_encode(lmrs_tokenizer* t, const char* text, size_t text_len, int bos, int eos, int chat_format, int model_type,
                          uint32_t* out, size_t cap, size_t* n);
int lmrs_tokenizer_decode(const lmrs_tokenizer* t, uint32_t token, char* out, size_t cap, size_t* n);
typedef struct lmrs_sampler lmrs_sampler;
int lmrs_sampler_create(uint32_t vocab_size, float temperature, float top_p, uint64_t seed, lmrs_sampler** out);
void lmrs_sampler_destroy(lmrs_sampler* s);
int lmrs_sampler_sample(lmrs_sampler* s, float* logits, uint32_t* next);
/* sample_topp (sampler.rs:67-106) from its sort on, for a caller that ran the temperature scaling, the softmax and the cutoff filter
 * elsewhere: pairs = n0 candidates {f32 prob, u32 index} with prob >= (1 - top_p) / (vocab_size - 1), in index order - what :74-80 leaves
 * in probindex[0 .. n0).  A stand-alone host entry point: the library itself goes through lmrs_sampler_exps_prepare / _finish. */
int lmrs_sampler_topp_pairs(lmrs_sampler* s, const void* pairs, size_t n0, uint32_t* next);
/* The same for a caller that has also sorted this call's n0 candidates: sorted_pairs by descending prob, ties in index order - exactly what the
 * stable sort of :81 makes of the index-ordered candidates (lmrs_batch_forward_sample sorts a flat row's candidates on the device).  The merge
 * with the stale rest of the persistent vector, the cumulative cut and the draw run here. */
int lmrs_sampler_topp_sorted_pairs(lmrs_sampler* s, const void* sorted_pairs, size_t n0, uint32_t* next);
/* The persistent candidate vector of a sampler, out and in, as it stands (host code): vocab_size pairs {f32 prob, u32 index}, 8 bytes each.
 * pairs may be NULL when only the flag is wanted.  *ordered (may be NULL): 1 when the vector is known to be in descending order of prob and free of NaNs - true from creation (all zeros) and after
 * every call of this library.  lmrs_sampler_set_candidates scans what it is given and sets that flag from what it finds; a vector that is not
 * ordered is sorted whole by every later call, as sampler.rs:81 writes it.  A sampler that takes another's vector continues exactly as the other
 * would.  set_candidates is refused between lmrs_sampler_exps_prepare and lmrs_sampler_exps_finish (this call's candidates sit in the vector). */
int lmrs_sampler_candidates(const lmrs_sampler* s, void* pairs, int* ordered);
int lmrs_sampler_set_candidates(lmrs_sampler* s, const void* pairs);
/* Sampler::sample from the softmax's exponentials on (functional.rs:134-139, then sampler.rs:119-128): exps[i] = exp(logits[i] / temperature - max)
 * were formed elsewhere (lmrs_forward_sample forms them on the device); the sequential sum, the division, and sample_mult / sample_topp run here.
 * exps become the probabilities in place.  Same token and probabilities as lmrs_sampler_sample on the logits. */
int lmrs_sampler_sample_exps(lmrs_sampler* s, float* exps, uint32_t* next);
/* The same in two halves, for a caller that sorts sample_topp's candidates itself (lmrs_forward_sample: on the device, when most of the vocabulary
 * passes the cutoff).  prepare: the sequential sum (functional.rs:134), the division (:137-139; exps become the probabilities in place) and, for a
 * top-p sampler, the cutoff filter of sampler.rs:71-80 - *n0 candidates are left in the sampler's vector in index order (0 for sample_mult).
 * finish: sorted_pairs = NULL: the reference's sort (:81) runs here; else the n0 candidates {f32 prob, u32 index} sorted by descending prob,
 * ties in index order - exactly what :81 makes of them; then the merge with the stale rest of the vector, the cumulative cut and the draw. */
int lmrs_sampler_exps_prepare(lmrs_sampler* s, float* exps, float* sum, float* cutoff, size_t* n0);
int lmrs_sampler_exps_finish(lmrs_sampler* s, const float* probs, const void* sorted_pairs, uint32_t* next);
int lmrs_sampler_info(const lmrs_sampler* s, uint32_t* vocab_size, float* temperature, float* top_p, float* rnd);   /* rnd = random_f32(seed), the same on every call (:119) */
/* Transformer::forward (src/transformer.rs:316) followed by Sampler::sample (src/sampler.rs:109-129) without the host ever touching the
 * logits: temperature 0 -> the argmax fused into the decode step; temperature != 0 -> the parallel part of the sampler on the device -
 * logits / temperature (:115), the maximum and exp(x - max) (functional.rs:126-133) - then the vocab_size exponentials cross to the host,
 * where lmrs_sampler_exps_prepare / _finish run the reference's sequential chains (the softmax sum, the running cdf) and sample_mult (:43-55) or
 * sample_topp (:67-106, the reference's default, chat.rs:28-31) over the sampler's persistent candidate vector; when more than 4096 candidates pass
 * the cutoff (a flat distribution) their sort (:81) runs on the device - a bitonic network over the unique keys (prob, index): the same permutation
 * as the reference's stable sort (7.05 -> 0.9 ms per token with 100 k candidates, profiles/r6_sampler_rate.txt).  Round 4 ran the chains
 * on the device as well (one wave, lane by lane): 1106 us per token against 1020 for the host sampler on copied logits - a dependent f32
 * add is ~1 ns on a host core and ~2.5 ns on one GPU lane; this split was measured at profiles/r5_sampler_rate.txt.  Same token as
 * lmrs_forward + lmrs_sampler_sample in every case.  One-GPU contexts (sharded ones copy the gathered logits). */
int lmrs_forward_sample(lmrs_ctx* ctx, uint32_t token, uint32_t pos, lmrs_sampler* sampler, uint32_t* next);
/* lmrs_batch_forward with a sampler per row (extension): ONE weight pass for n rows (1 .. 16), row i = Transformer::forward(tokens[i], pos[i]) on
 * slot[i]'s cache followed by Sampler::sample (sampler.rs:109-129) with samplers[i].  next[i] is, bit for bit, what lmrs_forward_sample returns for
 * that sampler on a context that holds only that sequence; the K/V rows are as lmrs_batch_forward leaves them; rows may mix samplers freely.
 * Temperature-0 rows take the pass's own argmax.  The others are sampled ON THE DEVICE, all rows at once: scaling, maximum and exponentials in
 * parallel; then the softmax sum and sample_mult's running cdf - one sequential f32 chain per row, which is why lmrs_forward_sample leaves them to
 * the host - as one chain per row side by side (16 rows cost the device the time of one, the host the time of 16); top-p rows leave their
 * candidates {prob, index} in index order.  ONE transfer brings back every row's token or candidate count and the first 4096
 * (LMRS_TOPP_DEVICE_SORT_MIN) candidates: 8 bytes a row for argmax / sample_mult rows instead of the vocab_size floats lmrs_batch_forward's logits
 * cost.  Top-p rows finish on the host in row order - lmrs_sampler_topp_pairs, each sampler's persistent vector updated exactly as that call
 * updates it; a row with 4096 candidates or more (a flat distribution) first has them sorted on the device (as lmrs_forward_sample does), one
 * such row at a time behind a second synchronise, and finishes through lmrs_sampler_topp_sorted_pairs.
 * lmrs_batch_generate, the device loop for argmax and sample_mult rows, is no device-resident sampled loop for top-p rows: sample_topp's stale
 * candidate vector lives in the host sampler, so a step with such a row cannot do without a host round trip - unless the vector itself goes to
 * the device, which is what lmrs_batch_generate_topp does for the length of a call.
 * Errors, each with a message of its own, before any device work, batch, context and samplers left usable: everything lmrs_batch_forward checks;
 * a NULL array; a NULL sampler (the row is named); a sampler made for another vocabulary size; a top-p sampler that appears twice in one call (it
 * carries state; argmax and sample_mult samplers are stateless and may be shared); a vocabulary whose last vocab_size % 4 logits the classifier
 * leaves unwritten.  A top-p row without a candidate fails the call with sample_topp's message and the row's number (the reference panics there).
 * The candidate buffers (16 * (vocab_size + 1) * 8 bytes on the device) are allocated at the first call with a sampled row, all or nothing. */
int lmrs_batch_forward_sample(lmrs_batch* b, uint32_t n, const uint32_t* slot, const uint32_t* tokens, const uint32_t* pos,
                              lmrs_sampler* const* samplers, uint32_t* next);
/* lmrs_batch_forward_runs with a sampler per run (extension): ONE weight pass over n_runs runs - the same runs, the same limits (1 .. lmrs_batch_width
 * runs, at most 512 rows, a slot in at most one run) - and the LAST row of every run whose samplers[i] is not NULL goes through Sampler::sample
 * (sampler.rs:109-129) with that sampler.  A NULL entry leaves the run's K/V rows only (a prompt chunk that is not the last) and next[i] = 0; when
 * every entry is NULL neither the final norm nor the classifier runs.  next[i] is, bit for bit, what lmrs_forward_sample returns for that sampler
 * after the run's tokens on a context that holds only that sequence; the K/V rows are as lmrs_batch_forward_runs leaves them; runs may mix argmax,
 * sample_mult and top-p samplers.  With runs of one token on a wide batch this is the sampled decode step of up to 64 sequences; with a prompt beside
 * the decode rows the prompt's first token is sampled in the pass that admits it.
 * The sampled rows go through lmrs_batch_forward_sample's six launches, up to the batch's width of them, and ONE transfer brings back every row's
 * token or candidate count and the first 4096 (LMRS_TOPP_DEVICE_SORT_MIN) candidates.  Top-p rows finish on the host in run order: a peaked row
 * through lmrs_sampler_topp_pairs; the rows with 4096 candidates or more (flat distributions) are first sorted on the device ALL TOGETHER - keys
 * straight from the candidates the filter left, one bitonic network with the row in the grid's second dimension, the rows padded to the power of two
 * that holds the longest - behind ONE second synchronise however many they are, and finish through lmrs_sampler_topp_sorted_pairs.  The host
 * finishes do not overlap the copies.  The device-resident loop that takes a top-p row is lmrs_batch_generate_topp (lmrs_batch_generate refuses one, for the reason given above).
 * Errors, each with a message of its own that opens with this call's name, before any device work, batch, context and samplers left usable:
 * everything lmrs_batch_forward_runs checks for these arguments; a NULL array; a sampler made for another vocabulary size (the run is named); a
 * top-p sampler in two runs of one call; a sampled (temperature != 0) output on a vocabulary whose last vocab_size % 4 logits the classifier leaves
 * unwritten; a logits block that holds fewer rows than the outputs asked for.  A top-p row without a candidate fails the call with sample_topp's
 * message and the run's number.
 * Buffers of this call's own, allocated at the first sampled call, all or nothing, the message gives the bytes: rows * (vocab_size + 1) * 8 bytes
 * of result blocks on the device for the sampled rows of the call in whole sixteens (made anew when a later call samples more rows), and from the
 * first call with a flat row F * N * 8 bytes of keys on the device and as many pinned (F flat rows, N the power of two >= their longest candidate
 * list, >= 8192; made anew when a call needs more: 64 MiB for 64 rows of a 128 k vocabulary).  lmrs_batch_forward_sample's buffers are not touched. */
int lmrs_batch_forward_runs_sample(lmrs_batch* b, uint32_t n_runs, const uint32_t* slot, const uint32_t* start_pos, const uint32_t* run_len,
                                   const uint32_t* tokens, lmrs_sampler* const* samplers, uint32_t* next);
/* ---- embedding rows in a batch (extensions): the rows of a pass need not be born from token ids.  The reference's multimodal chat loop
 * (src/bin/chat.rs:84-121) splices the image features of PHI3VProcessor::forward between two get_embeddings blocks and hands the rows to
 * Transformer::fill_kv_cache (transformer.rs:672-684), which runs forward_layer (:388-657) over them as they are.  The three calls below do that
 * on a batch slot; the layers never look at where a row came from, so only the source of the rows differs from the token calls. */
/* == lmrs_fill_kv_cache(embeddings, n, start_pos) on a context that holds only slot's sequence: ONE fill_kv_cache call of the reference
 * (transformer.rs:672-684; forward_layer, :388-657) run into slot's cache.  embeddings: n rows of dim floats (fill_kv_cache's `embeddings`), taken as
 * given - no sqrt(dim) scale on Gemma-2 - and never written; n: fill_kv_cache's `n`; start_pos: its `curr_pos`.  Gemma-2's 4096-key window is tested
 * against start_pos for EVERY row, as one forward_layer(sl = n) call tests it (the u32 `pos - t` of transformer.rs:525) and as lmrs_fill_kv_cache does.
 * The rows go 512 at a time through the batched pass (the skinny form below 16 rows; one row through the long table's pass).  residual (n*dim, may
 * be NULL): what the reference leaves in its mutated argument, the residual stream behind the last layer; NULL: nothing is downloaded, which is what
 * this call saves over lmrs_fill_kv_cache + lmrs_batch_fork.  Q4_0 files with n > 1 give the token-by-token values, the documented deviation of
 * lmrs_fill_kv_cache.  The context's own cache and the other slots are untouched.
 * Errors, each with a message of its own that opens with this call's name, before any device work, batch and context left usable: a NULL batch or
 * embeddings, n == 0, slot >= n_slots, start_pos + n > seq_len.  Non-finite values in the rows are not an error: the reference does not check them. */
int lmrs_batch_prefill_embeddings(lmrs_batch* b, uint32_t slot, const float* embeddings /* n*dim */, uint32_t n,
                                  uint32_t start_pos, float* residual /* n*dim, may be NULL */);
/* lmrs_batch_forward_runs with a kind per run: run_kind[i] = 0, run i is a token run, exactly a run of lmrs_batch_forward_runs; 1, an EMBEDDING run -
 * row j of it is fill_kv_cache(&row, 1, start_pos[i] + j) (transformer.rs:672-684; forward_layer, :388-657) on a context that holds only that
 * sequence: the row is taken as given (no sqrt(dim) scale on Gemma-2), Gemma-2's window is tested against the row's OWN position, the rest is the
 * chain every row of the pass shares.  This differs from lmrs_batch_prefill_embeddings - ONE fill_kv_cache(n) call, the window on its first position -
 * only on Gemma-2 past 4096 positions.
 *   tokens: one id per row of the TOKEN runs only, packed in run order; embeddings: dim floats per row of the EMBEDDING runs only, packed in run
 *   order, never written; either may be NULL when the call has no run of its kind.
 * An embedding run may ask for outputs (n_out): its rows then go through the final norm and the classifier like any other row - on Llama / Phi the
 * tail of Transformer::forward (transformer.rs:316-384), on Gemma-2 with both soft caps, as for token rows.  All limits are lmrs_batch_forward_runs'
 * own: at most 512 rows, at most lmrs_batch_width runs, a slot in at most one run; outputs, K/V rows and stale rows as that call documents them.
 * With run_kind all zero the results are bit for bit lmrs_batch_forward_runs' (the same launches).  A call with an embedding run uploads the rows
 * into a [512][dim] f32 block on the device (allocated at the first such call, all or nothing, the message gives the bytes) and ONE launch,
 * source_rows_kernel, stands where the token rows' dequantisation stands: per row the token's embedding with that launch's exact arithmetic, or a
 * copy of the staged row.
 * Errors, each with a message of its own that opens with this call's name, before any device work, batch and context left usable: everything
 * lmrs_batch_forward_runs checks; a run_kind other than 0 or 1 (the run is named); tokens NULL with a token run present; embeddings NULL with an
 * embedding run present.  Non-finite values in the rows are not an error. */
int lmrs_batch_forward_runs_embed(lmrs_batch* b, uint32_t n_runs, const uint32_t* slot, const uint32_t* start_pos, const uint32_t* run_len,
                                  const uint32_t* n_out, const uint32_t* run_kind /* 0 tokens, 1 embeddings */, const uint32_t* tokens,
                                  const float* embeddings, uint32_t* argmax, float* logits,
                                  uint32_t k, uint32_t* topk_idx, float* topk_logprob);
/* lmrs_batch_forward_runs_sample with a kind per run: run_kind, tokens and embeddings as lmrs_batch_forward_runs_embed takes them (row j of an
 * embedding run = fill_kv_cache(&row, 1, start_pos[i] + j), transformer.rs:672-684; forward_layer, :388-657), samplers and next as
 * lmrs_batch_forward_runs_sample takes them: the last row of an embedding run that has a sampler is sampled like a token run's.  With run_kind all
 * zero next and the samplers' states are bit for bit lmrs_batch_forward_runs_sample's.  Errors: everything that call checks, and the three of
 * lmrs_batch_forward_runs_embed, each message opening with this call's name, before any device work; batch, context and samplers left usable. */
int lmrs_batch_forward_runs_embed_sample(lmrs_batch* b, uint32_t n_runs, const uint32_t* slot, const uint32_t* start_pos, const uint32_t* run_len,
                                         const uint32_t* run_kind, const uint32_t* tokens, const float* embeddings,
                                         lmrs_sampler* const* samplers, uint32_t* next);
/* The sort of lmrs_batch_forward_runs_sample's flat rows on caller-supplied candidates, ONE call of its launcher: pairs = n_rows (1 .. 64) rows of ld
 * (1 .. 2^24) entries {f32 prob >= 0, u32 index}, the first n0[r] (<= ld) of row r in ascending index order.  sorted (n_rows x ld): row r's first
 * n0[r] entries by descending prob, ties by ascending index - what the stable sort of sampler.rs:81 makes of them; the rest of the row, and a row
 * with n0 = 0, is not written.  Everything else is refused before the device is touched. */
int lmrs_op_sort_candidates(int device, const void* pairs, size_t n_rows, size_t ld, const uint32_t* n0, void* sorted);
/* The launches that finish a top-p row on the device (lmrs_batch_generate_topp) on caller-supplied rows: unit parity against lmrs_sampler_topp_pairs.
 * Row r < n_rows (1 .. 64) over n (2 .. 2^24) entries: cand + r * n pairs holds its n0[r] (<= n) candidates {f32 prob > 0, u32 index} in ascending index
 * order, state + r * n pairs its persistent vector in descending order of prob, top_p[r] and rnd[r] its parameters.  Afterwards state holds the new
 * vector - the candidates sorted by (prob descending, index ascending) and merged stably with entries [n0, n) of the old one, equal probabilities from
 * the candidates first: what sampler.rs:81 leaves - token[r] the draw of sampler.rs:83-105 and status[r] = 0; n0[r] == 0: status[r] = 1, token[r] = 0,
 * the state unchanged.  Everything else is refused before the device is touched. */
int lmrs_op_topp_rows(int device, size_t n_rows, size_t n, const void* cand, const uint32_t* n0, const float* top_p, const float* rnd,
                      void* state, uint32_t* token, uint32_t* status);

/* ---- allowed-token masks: which tokens a slot's rows may produce (extensions, no reference counterpart) ----
 * A mask is state of a batch slot, not an argument of a pass: W = (vocab_size + 31) / 32 words, bit (t & 31) of word (t >> 5) set = token t allowed;
 * bits at and above vocab_size are ignored.  While slot s has a mask, every output row of s in any batch call - lmrs_batch_forward, _generate_greedy
 * (every one of its steps, the mask constant over them), _forward_runs (all n_out rows of the run), _forward_sample, _forward_runs_sample and the two
 * _embed forms, contiguous or paged - is computed from the row's logits with the disallowed entries equal to -inf: the logits the caller downloads
 * show -inf exactly at the cleared bits and the unmasked bits everywhere else, argmax is sample_argmax (sampler.rs:29-41) of that row, the top-k
 * the k first candidates of it, a sampled token Sampler::sample (sampler.rs:109-129) of it - temperature-0 samplers included.  No floating-point
 * operation on an allowed logit changes.  One launch (mask_rows_kernel) behind the classifier and Gemma's soft-cap writes the -inf, for the slabs of
 * logits rows that have a masked row; a batch on which no mask was set, or all were cleared, runs exactly the launches it ran without this call.
 * A mask touches no K/V row, no other slot, no call of the context's own and no row without outputs.  It stays until it is replaced or cleared:
 * lmrs_batch_fork and lmrs_batch_release neither copy nor clear it.
 * lmrs_batch_set_masks: the masks of n slots (mask i = bits + i * W, for slot[i]), ordered before the next pass; the caller's arrays are free on return.
 *   One copy uploads all n.  The device block (n_slots x W words) and a pinned block of the same size are allocated at the first call, all or nothing
 *   (the message gives the bytes); lmrs_batch_destroy frees them.  n == 0 does nothing.
 * lmrs_batch_clear_masks: the slots named lose their masks; n == 0 (slot may be NULL): every slot.  A slot without a mask is not an error.
 * lmrs_batch_mask_info: *n_allowed = the tokens below vocab_size the slot's mask allows; 0: the slot has no mask.
 * Errors, each with a message of its own that opens with the call's name, before any device work, batch, context and samplers left usable: a NULL
 * batch; a NULL array with n > 0; n above lmrs_batch_width; a slot >= n_slots; the same slot twice in one call; a mask with no allowed token below
 * vocab_size (the slot is named); a model whose classifier leaves a tail of the vocabulary unwritten (the sampled calls' condition).
 * lmrs_batch_forward_runs and lmrs_batch_forward_runs_embed refuse k > n_allowed of a masked slot that has outputs in the call (the message gives
 * the slot, k and n_allowed): such a row has only n_allowed candidates that are numbers. */
int lmrs_batch_set_masks(lmrs_batch* b, uint32_t n, const uint32_t* slot, const uint32_t* bits /* n * W */);
int lmrs_batch_clear_masks(lmrs_batch* b, uint32_t n, const uint32_t* slot);
int lmrs_batch_mask_info(const lmrs_batch* b, uint32_t slot, uint32_t* n_allowed /* 0: no mask */);

/* ---- repetition, presence and frequency penalties per slot, over a token record kept on the device (extensions, no reference counterpart) ----
 * The record: hist[n_slots][seq_len] words on the device, hist[s][p] = the token whose K/V row stands at position p of slot s, LMRS_TOKEN_NONE where it
 * is unknown or the row was an embedding.  It is made - all NONE - by the first lmrs_batch_set_history or lmrs_batch_set_penalties call (all or
 * nothing, the message gives the bytes) and until then a batch enqueues exactly the launches and copies it enqueued without these calls.  From then
 * on every batch call that writes K/V rows of a slot writes the record of the same positions: lmrs_batch_forward, _forward_sample, _forward_runs* and
 * every step of lmrs_batch_generate_greedy (one launch over the pass's device table, so the loop's own tokens are recorded without crossing to the
 * host), lmrs_batch_prefill (contiguous and paged); lmrs_batch_prefill_embeddings and embedding runs write NONE; lmrs_batch_fork copies the first
 * n_pos entries of src to dst, NONE from LMRS_BATCH_CTX.  The record is a function of the position, not a counter: a position is rewritten before it
 * is read again, so rewinds, rejected drafts and lmrs_batch_release need no bookkeeping.
 * The rule.  Output row r of slot s at position p, logits l (f32) as the classifier and Gemma's soft-cap leave them; H = the entries hist[s][i],
 * 0 <= i <= p, that are not NONE (the row's own input token is one of them); c_all[t] = occurrences of t in H, c_out[t] = those at i >= out_from[s]:
 *   for every t with c_all[t] > 0 and repetition != 1:  l[t] = l[t] > 0 ? l[t] / repetition : l[t] * repetition
 *   then for every t with c_out[t] > 0:                   l[t] = (l[t] - frequency * (float)c_out[t]) - presence
 * each operation one correctly rounded f32 operation (the division IEEE), nothing contracted; no other logit changes; the counts are integers, so the
 * result does not depend on scheduling.  The slot's mask is applied behind this and the sinks run unchanged: the logits a caller downloads, argmax,
 * top-k, log-probabilities and sampled tokens of every batch call, contiguous, wide or paged, come from the penalised row.  repetition < 1 and
 * negative presence / frequency are legal (they raise seen tokens); (1, 0, 0) is the same as clearing.  Penalties stay until replaced or cleared:
 * lmrs_batch_fork and lmrs_batch_release neither copy nor clear them.  The context's own calls (lmrs_forward*, lmrs_generate_*) are not touched.
 * lmrs_batch_set_history: hist[slot][start_pos .. start_pos + n) = tokens (what a caller knows of positions written before the record existed);
 *   n may be 0: only switches the record on.  lmrs_batch_history: the same range read back; an error while the batch keeps no record.
 * lmrs_batch_set_penalties: the parameters of n slots (arrays of n); lmrs_batch_clear_penalties: n == 0 (slot may be NULL): every slot;
 * lmrs_batch_penalty_info: the slot's parameters as set ((1, 0, 0, 0) if never), *active = 1 while they change a logit.
 * Errors, each with a message that opens with the call's name, before any state changes: a NULL batch; a NULL array with n > 0; n above
 * lmrs_batch_width; a slot >= n_slots; the same slot twice in one call; a value that is not finite; repetition <= 0; out_from > seq_len; a token
 * >= vocab_size that is not LMRS_TOKEN_NONE; start_pos + n > seq_len; a model whose classifier leaves a tail of the vocabulary unwritten. */
#define LMRS_TOKEN_NONE 0xFFFFFFFFu
int lmrs_batch_set_history(lmrs_batch* b, uint32_t slot, uint32_t start_pos, const uint32_t* tokens, size_t n);
int lmrs_batch_history(lmrs_batch* b, uint32_t slot, uint32_t start_pos, size_t n, uint32_t* out);
int lmrs_batch_set_penalties(lmrs_batch* b, uint32_t n, const uint32_t* slot, const float* repetition, const float* presence,
                             const float* frequency, const uint32_t* out_from);
int lmrs_batch_clear_penalties(lmrs_batch* b, uint32_t n, const uint32_t* slot);
int lmrs_batch_penalty_info(const lmrs_batch* b, uint32_t slot, float* repetition, float* presence, float* frequency,
                            uint32_t* out_from, int* active);

/* ---- the device loop whose rows end one by one: stop sets, budgets, samplers, log-probabilities (extension) ----
 * lmrs_batch_generate_greedy with the loop's own control.  Row i starts with t_0 = tokens[i]; for j = 0, 1, ...:
 *   1. Transformer::forward(t_j, pos[i] + j) runs on slot[i];
 *   2. o_j is chosen from the row as the sinks see it - the slot's penalties, then its mask, exactly as in every other batch call - by
 *      Sampler::sample (sampler.rs:109-129) with samplers[i], or Sampler::sample_argmax (:29-41) for a NULL entry (samplers NULL: every row);
 *   3. out_tokens[i*M + j] = o_j, M = the largest max_new of the call;
 *   4. o_j in row i's stop set: the row ends, finish[i] = LMRS_FINISH_STOP;
 *   5. else j + 1 == max_new[i]: the row ends, finish[i] = LMRS_FINISH_BUDGET;
 *   6. else t_{j+1} = o_j.
 * n_out[i] = j + 1 at the end.  STOP wins when both hold; the stop token is reported and never fed (the loop of chat.rs:188-222 on EOS).
 * Every token is, bit for bit, what the per-sequence calls give - lmrs_forward_argmax or lmrs_forward_sample on a context that holds only that
 * sequence; with no stop sets, NULL samplers and equal budgets out_tokens is lmrs_batch_generate_greedy's.  Results do not depend on check_every.
 * A finished row leaves its slot exactly as n_out[i] feeds leave it: K/V rows and record entries pos[i] .. pos[i] + n_out[i] - 1 are written, and
 * no K/V row, record entry or page-table entry at or beyond pos[i] + n_out[i] changes through the row's own progress.  On a paged batch the pages
 * of [pos[i], pos[i] + max_new[i]) are claimed up front, per row, all or nothing, under the accounting of every other call; the pages an early stop
 * did not reach stay with the slot, cleared, until lmrs_batch_release(slot, pos[i] + n_out[i]) gives them back.
 * Stop sets: n_stop[i] <= LMRS_STOP_MAX tokens of row i, packed in row order in stop_tokens (n_stop NULL: no row has one).
 * Samplers: argmax (temperature 0) and sample_mult (top_p <= 0 or >= 1) samplers; being stateless they may be shared between rows (the reference never
 * advances its seed, sampler.rs:119, so the loop carries no generator state).  A top-p sampler is refused, the row named: sample_topp's stale candidate
 * vector lives in the host sampler (sampler.rs:81), so a step with such a row cannot do without a host round trip.  Sampled rows: up to the batch's width.
 * out_logprobs (may be NULL: the loop then enqueues nothing for it), same layout as out_tokens: the log-softmax of that same row (penalised, masked,
 * temperature 1) at o_j by lmrs_score_tokens' definition - the f32 maximum widened to double, the sum in double over all vocabulary entries, one
 * rounding to float.  Entries beyond n_out[i] of both blocks are written as 0.
 * The loop: check_every passes are enqueued, each followed by ONE launch that records the chosen tokens, tests them against the stop sets and budgets
 * and moves the live rows on; then the host reads the rows' states and goes on with a table of the live rows alone (the pass forms follow the row
 * count as in every call: 17 rows and more the long table, fewer the 16-row table).  A row that has ended inside a chunk computes its last row again -
 * the same bits into the same places.  stats2 (may be NULL): [0] = passes run = the largest ceil(n_out[i] / check_every) * check_every, [1] = the sum
 * over the passes of the rows in the pass = the sum over rows of that quantity.  *seconds (may be NULL): host wall time of the call.
 * Errors, each with a message of its own that opens with the call's name, before any device work, batch, context and samplers left usable:
 * everything lmrs_batch_generate_greedy checks, with pos[i] + max_new[i] against seq_len; a NULL required array; max_new[i] == 0; n_stop[i] >
 * LMRS_STOP_MAX; n_stop given without stop_tokens; a stop token >= vocab_size; check_every == 0; a top-p sampler; a sampler for another vocabulary
 * size; a sampled row, or out_logprobs, on a model whose classifier leaves a vocabulary tail unwritten (or with more rows than the logits block
 * holds); too few free pages - the message gives the pages wanted and the pages free, and nothing has changed.
 * Buffers of this call's own, allocated at first need, all or nothing: the rows' state blocks; n * M floats (and as many pinned) for
 * out_logprobs, made anew when a call needs more; rows * (vocab_size + 1) * 8 bytes of result blocks for sampled rows in whole sixteens, and rows * vocab_size floats more when sampled
 * rows and out_logprobs meet (the samplers then work on a copy of the logits).  The buffers of the other sampled calls are not touched. */
#define LMRS_STOP_MAX 16
enum { LMRS_FINISH_BUDGET = 0, LMRS_FINISH_STOP = 1 };
int lmrs_batch_generate(lmrs_batch* b, uint32_t n, const uint32_t* slot, const uint32_t* tokens, const uint32_t* pos,
                        const uint32_t* max_new, const uint32_t* n_stop, const uint32_t* stop_tokens, lmrs_sampler* const* samplers,
                        uint32_t check_every, uint32_t* out_tokens, float* out_logprobs, uint32_t* n_out, uint32_t* finish,
                        uint64_t* stats2, double* seconds);

/* ---- lmrs_batch_generate with top-p rows: the candidate vectors resident on the device for the length of the call (extension) ----
 * lmrs_batch_generate's contract word for word - arguments, outputs, stop sets, budgets, log-probabilities, masks, penalties, contiguous, wide and
 * paged batches, any check_every, stats2, errors (each message opens with this call's name) - with these differences:
 *   - a top-p sampler (temperature != 0, 0 < top_p < 1: the reference's default, chat.rs:28-31) is accepted for a row; rows may mix argmax,
 *     sample_mult and top-p samplers.  A top-p sampler carries state from call to call and may appear in one row only;
 *   - every token is, bit for bit, what lmrs_forward_sample returns with that sampler on a context that holds only that sequence, stale entries of the
 *     sampler's persistent vector included (sampler.rs:81 sorts the whole vector);
 *   - when the call returns, every top-p sampler's host vector is, bit for bit, what n_out[i] such per-sequence calls leave in it: whatever the caller
 *     does with the sampler next continues exactly;
 *   - a row whose step finds no candidate above the cutoff (the reference underflows n0 - 1 and panics there, lmrs_sampler_topp_pairs fails the call)
 *     ends with finish[i] = LMRS_FINISH_NO_CANDIDATE.  That step reports no token: n_out[i] counts the tokens before it and may be 0.  Its K/V row and
 *     record entry are written - the forward ran - and the sampler's vector is as the steps before it left it (the sort of an unchanged ordered vector
 *     changes nothing).  The call returns 0 and the other rows go on;
 *   - a top-p sampler whose vector is not ordered (lmrs_sampler_candidates: an import through lmrs_sampler_set_candidates) is refused before any device
 *     work, with a message of its own: the device merge rests on the order every call of this library leaves.
 * The device side: the vectors travel to the device at the start of the call (one that is still all zero, as created, is cleared there instead) and
 * back through lmrs_sampler_set_candidates at its end; they do not stay resident between calls.  Behind launch_sample_rows' six launches every pass with
 * a live top-p row enqueues a fixed sequence - its length set by vocab_size alone, no n0 known to the host: the bitonic sort of each row's n0 candidates
 * on the keys (~bits(prob) << 32) | index, sized per row on the device (a row of up to 8192 candidates is done after the first launch, the others
 * return at once); the stable merge with the ordered rest of the vector by rank, one binary search per element, into the row's second block
 * (ping-pong; only the prefix that changes is written: a few hundred bytes for a peaked row, up to 2 * vocab_size * 8 read and written for a flat
 * one); the cumulative cut and the draw, one adding lane per row.  A row that has ended but still stands in the table reads its live word and leaves
 * its vector alone.  The vectors are addressed by the row's number among the call's top-p rows, a column beside the pass's table: no vector moves
 * when the table is rebuilt.
 * Measured on Llama-3.2-1B Q8_0 (synthetic weights, rows at 100 positions, 128 tokens, upload and download included) against one
 * lmrs_batch_forward_runs_sample per step: flat rows (0.7, 0.9) 4073 against 13047 us a step at 64 rows, 2895 against 4136 at 16; peaked rows
 * (0.02, 0.9) 1780 against 1863 at 16 rows, but 2346 against 2294 at 64 - slower by 52 us a step there.  The new launches alone: 113 us a step for 64
 * peaked rows, 2063 us for 64 rows of 112224 candidates (profiles/batch_generate_topp_llama1b.txt).
 * Gemma-2-2B Q4_0: flat rows 9150 against 25602 us at 64 rows, 5866 against 9058 at 16; peaked rows slower at both sizes, 3744 against 3714 and 5632
 * against 5454 (profiles/batch_generate_topp_gemma2b_q4.txt): five of the eight cases are no slower than the per-call route, three are slower.
 * Buffers of this call's own beside lmrs_batch_generate's, at the first call that needs them, all or nothing, the bytes in the message: per top-p row
 * 2 * vocab_size * 8 bytes of vector blocks, 8 bytes times the power of two that holds max(vocab_size, 8192) of sort keys, and vocab_size * 8 pinned. */
#define LMRS_FINISH_NO_CANDIDATE 2
int lmrs_batch_generate_topp(lmrs_batch* b, uint32_t n, const uint32_t* slot, const uint32_t* tokens, const uint32_t* pos,
                             const uint32_t* max_new, const uint32_t* n_stop, const uint32_t* stop_tokens, lmrs_sampler* const* samplers,
                             uint32_t check_every, uint32_t* out_tokens, float* out_logprobs, uint32_t* n_out, uint32_t* finish,
                             uint64_t* stats2, double* seconds);

/* ---- token automata on batch slots: a mask that follows the chosen token, inside the device loops (extensions, no reference counterpart) ----
 * A grammar needs another mask after every token; lmrs_batch_set_masks' mask is constant over a call.  An automaton is a DFA over tokens in the usual
 * compressed form: class_of[vocab_size] (uint16_t, each below n_classes), next[n_states * n_classes] (each a state or LMRS_STATE_DEAD), and an optional
 * final flag per state (final NULL: no state is final).  Token t is allowed in state q iff next[q][class_of[t]] != DEAD, and choosing t moves the slot to
 * that state.  Every state that is not final must allow at least one token below vocab_size; a final state may allow none.
 * Host only, plain arithmetic, no device touched:
 * lmrs_automaton_check: the tables' rules - n_states in 1 .. 2^31 - 1, n_classes in 1 .. 65536, every class below n_classes (the token and the class are
 *   named), every next entry a state or DEAD (the state and the class are named), every non-final state with an allowed token (the state is named; where
 *   its live classes are all empty, the first of them too); n_allowed_out (n_states words, may be NULL): the allowed tokens of every state.
 * lmrs_automaton_walk: tokens[0 .. n) from `state`; 0, *out_state = the state behind them, *n_walked = n.  At the first token its state does not allow the
 *   call fails (the message names the token and the state) with *n_walked = the tokens consumed and *out_state = the state in front of that token.
 * Automata of a batch, at most LMRS_AUTOMATA_MAX (16) at a time:
 * lmrs_batch_automaton_create: runs the check (under this call's name), uploads class_of and next - the final flag folded into bit 31 of the next entries,
 *   so the step boundary needs no third dependent load - and BUILDS THE PER-STATE MASKS ON THE DEVICE (automaton_masks_kernel): n_states * W words in
 *   lmrs_batch_set_masks' bit layout, bits at and above vocab_size clear.  2 * vocab_size + 4 * n_states * (n_classes + W) bytes on the device, all or
 *   nothing, the message gives the bytes; the caller's arrays are free on return.  Refused on a model whose classifier leaves a vocabulary tail unwritten.
 * lmrs_batch_automaton_destroy: refused while a slot is attached to it; lmrs_batch_destroy frees every automaton of the batch.
 * lmrs_batch_attach_automaton: slot[i] is attached to a[i] in state[i] (a[i] NULL: detached, state[i] ignored; detaching a slot without one is no error).
 * lmrs_batch_automaton_state: the slot's state, that state's allowed tokens and its final flag; *state = LMRS_STATE_DEAD (the others 0): no automaton.
 * lmrs_batch_automaton_advance: lmrs_automaton_walk applied to the slot's state; a disallowed token fails the call and changes nothing.
 * lmrs_op_automaton_masks: the mask builder alone on caller-supplied tables (bits_out: n_states * W words); the tables' ranges are checked, the rule
 *   about non-final states is not.
 * Semantics, in the masks' own words: a slot with an automaton has, at every moment, the mask of its current state.  Every output row of the slot in any
 * batch call - lmrs_batch_forward, _forward_runs* (all n_out rows under the slot's current state: a draft is verified under it), _forward_sample,
 * _forward_runs_sample, the _embed forms and both device loops, contiguous, wide and paged - is computed under that mask, behind the slot's penalties and
 * in front of every sink, bit for bit as lmrs_batch_set_masks defines it.  The launch (auto_rows_mask_kernel) is mask_rows_kernel with the row's mask
 * address resolved on the device through the slot's state word: masks + state * W.  ONLY the explicit calls above and the two device loops move a state.
 * lmrs_batch_mask_info reports the current state's count, lmrs_batch_forward_runs refuses k above it; lmrs_batch_fork and lmrs_batch_release neither copy
 * nor clear an attachment.  A batch that never attaches an automaton enqueues exactly what it enqueued without these calls.
 * The device loops (lmrs_batch_generate, lmrs_batch_generate_topp; signatures unchanged).  Steps 1 to 6 run as documented; the boundary launch also forms
 * q' = next[q][class_of[o_j]] for every live row whose slot has an automaton, and between STOP and BUDGET stands a new ending: q' final - the row ends
 * with finish[i] = LMRS_FINISH_FINAL, the token reported and never fed.  A row that stays live has q' stored in the slot's state word on the device, and
 * the next pass is masked under it with no host involvement (nor does a rebuilt table need anything new: it names slots, not states).  A row that ends
 * leaves its state word alone, so its recomputed last row is the same bits into the same places; the host completes the walk when it collects the row:
 * when the call returns, lmrs_batch_automaton_state of every row's slot is the walk of its n_out reported tokens from the start state (a STOP or BUDGET
 * token included; a LMRS_FINISH_NO_CANDIDATE step reports no token and moves nothing).  Results do not depend on check_every; out_logprobs come from the
 * masked row; stats2, the paged claims and "no write beyond pos + n_out" are unchanged.  A row whose allowed logits hold no number can choose a token
 * its state does not allow: the device leaves such a state alone and the call fails at the end with the walk's message.
 * Not measured yet: the loop against one set_masks + one-token lmrs_batch_generate per step, and the automaton's cost per pass (DESIGN.md 4.4.15;
 * hostcpp/batch_grammar.cpp prints both).
 * Errors, each with a message of its own that opens with the call's name, before any device work, the states unchanged, batch and context usable:
 * a NULL batch or array; a handle that is not an automaton of this batch; a seventeenth automaton; slot >= n_slots, the same slot twice, n above
 * lmrs_batch_width; attaching to a slot that has a mask, and lmrs_batch_set_masks on a slot that has an automaton (one mask source per slot: a ban-list
 * belongs in the automaton's classes); a start state out of range; a start state that is final and allows no token; any pass whose output rows include
 * a slot standing in a final state that allows no token; lmrs_batch_generate_greedy with a row whose slot has an automaton (lmrs_batch_generate without
 * stop sets is its superset). */
#define LMRS_STATE_DEAD 0xFFFFFFFFu
#define LMRS_AUTOMATA_MAX 16
#define LMRS_FINISH_FINAL 3
typedef struct lmrs_automaton lmrs_automaton;
int lmrs_automaton_check(uint32_t vocab_size, uint32_t n_states, uint32_t n_classes, const uint16_t* class_of, const uint32_t* next,
                         const uint8_t* final /* n_states, may be NULL */, uint32_t* n_allowed_out /* n_states, may be NULL */);
int lmrs_automaton_walk(uint32_t vocab_size, uint32_t n_states, uint32_t n_classes, const uint16_t* class_of, const uint32_t* next,
                        const uint8_t* final, uint32_t state, const uint32_t* tokens, size_t n, uint32_t* out_state, size_t* n_walked);
int lmrs_batch_automaton_create(lmrs_batch* b, uint32_t n_states, uint32_t n_classes, const uint16_t* class_of, const uint32_t* next,
                                const uint8_t* final, lmrs_automaton** a);
int lmrs_batch_automaton_destroy(lmrs_batch* b, lmrs_automaton* a);
int lmrs_batch_attach_automaton(lmrs_batch* b, uint32_t n, const uint32_t* slot, lmrs_automaton* const* a /* a[i] NULL: detach */, const uint32_t* state);
int lmrs_batch_automaton_state(const lmrs_batch* b, uint32_t slot, uint32_t* state /* LMRS_STATE_DEAD: no automaton */, uint32_t* n_allowed, int* is_final);
int lmrs_batch_automaton_advance(lmrs_batch* b, uint32_t slot, const uint32_t* tokens, size_t n);
int lmrs_op_automaton_masks(int device, uint32_t vocab_size, uint32_t n_states, uint32_t n_classes, const uint16_t* class_of, const uint32_t* next,
                            uint32_t* bits_out /* n_states * W */);

/* ---- candidate filters per slot: top_k and min_gap (min_p in logit space), applied on the device (extensions, no reference counterpart) ----
 * The rule.  Output row r of slot s, logits l[0 .. vocab_size) (f32) as they stand BEHIND Gemma's soft-cap, the slot's penalties and its mask or its
 * automaton's mask; the slot's parameters top_k (0: off) and min_gap (+inf: off):
 *   1. the candidate order is lmrs_score_tokens_topk's: the larger value first, -0.0 equal to +0.0, equal values by ascending index, a NaN behind every
 *      number (NaNs by ascending index) but a NaN at index 0 first of all.  m = the value of the first candidate.
 *   2. if top_k != 0 and top_k < vocab_size: every entry that is not among the first top_k candidates becomes -inf.
 *   3. if min_gap is finite: thr = m - min_gap, one correctly rounded f32 subtraction; every entry with !(l[t] >= thr) becomes -inf (a NaN entry too).  If m
 *      is a NaN this step clears nothing.  Every value tied at thr stays: this step never looks at indices.
 *   4. no kept logit is changed by any floating-point operation; entries that are -inf already stay; the first candidate is always kept.
 * The k-th candidate is found exactly for any top_k, by integer counts: the result does not depend on scheduling.  The sinks run unchanged on the filtered
 * row: downloaded logits show -inf exactly at the cut entries; argmax is unchanged; top-k outputs and ranks are those of the filtered row (candidates beyond
 * the kept set are its -inf entries in index order, log-probability -inf); sampled tokens (sample_mult, top-p) and every log-probability - lmrs_batch_forward_runs'
 * and lmrs_batch_generate's out_logprobs - are the filtered row's: the chosen token's log-probability is RENORMALISED over the kept set, as under a mask.
 * A caller turns min_p into min_gap = -temperature * ln(min_p) (a token stays while its probability is at least min_p times the largest): the library never
 * sees min_p, so the result is defined in logit space and is bit-exact.
 * Filters are state of a slot: they stay until replaced or cleared; lmrs_batch_fork and lmrs_batch_release neither copy nor clear them; they touch no K/V
 * row, no other slot and no call of the context's own (lmrs_forward*, lmrs_generate_*), and they are constant over a device-loop call.
 * lmrs_batch_generate_greedy SKIPS the launch: no filter moves an argmax.  A batch on which no filter was ever switched on enqueues exactly the launches
 * and copies it enqueued without these calls.
 * lmrs_batch_set_filters: the parameters of n slots (arrays of n); (0, +inf) is the same as clearing; top_k >= vocab_size is legal and inactive.
 * lmrs_batch_clear_filters: n == 0 (slot may be NULL): every slot.
 * lmrs_batch_filter_info: the slot's parameters as set ((0, +inf) if never), *active = 1 while they can clear a logit.
 * lmrs_op_filter_rows: the kernel alone on n_rows caller rows of n logits at stride ld, in place (host memory; the floats between rows come back as they
 *   went); a row with top_k 0 or >= n and min_gap +inf is left alone.  1 <= n_rows <= 65535, 1 <= n <= ld <= 2^24.
 * Errors, each with a message that opens with the call's name, before any state changes: a NULL batch; a NULL array with n > 0; n above lmrs_batch_width;
 * a slot >= n_slots; the same slot twice in one call; a min_gap that is NaN or negative; a model whose classifier leaves a tail of the vocabulary unwritten. */
int lmrs_batch_set_filters(lmrs_batch* b, uint32_t n, const uint32_t* slot, const uint32_t* top_k /* n */, const float* min_gap /* n */);
int lmrs_batch_clear_filters(lmrs_batch* b, uint32_t n, const uint32_t* slot);
int lmrs_batch_filter_info(const lmrs_batch* b, uint32_t slot, uint32_t* top_k, float* min_gap, int* active);
int lmrs_op_filter_rows(int device, float* rows, size_t n_rows, size_t n, size_t ld, const uint32_t* top_k /* n_rows */, const float* min_gap /* n_rows */);

#ifdef __cplusplus
}
#endif
#endif /* LMRS_HIP_H */
