// transformer.hpp — C++ host-side mirror of lmrs::transformer::Transformer over the C ABI.
//
// The reference is compiled code (Rust) and its toolchain is absent from the build image, so the host
// layer above the C ABI is provided in C++ with the reference's names, argument meaning and error
// behaviour (reference src/transformer.rs:127-131 struct, :134 new, :316 forward, :659 get_embeddings,
// :672 fill_kv_cache; errors there are panics -> here exceptions).  Header-only; link liblmrs_hip.so.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../../include/lmrs_hip.h"

namespace lmrs_host {

struct Panic : std::runtime_error { using std::runtime_error::runtime_error; };
inline void check(int rc) { if (rc != 0) throw Panic(lmrs_last_error()); }

using TransformerArgs = lmrs_args;

// Unit-parity aid: the stream GEMM of a batch pass of 17 .. 47 rows on caller-supplied operands, here at any 1 <= n_tok <= 64  (lmrs_debug_gemm_wide)
inline std::vector<float> debug_gemm_wide(const std::int8_t* xq, const float* xs, const std::uint8_t* wq, const float* ws, std::size_t n, std::size_t o,
                                          std::size_t n_tok, bool q4, int device = 0) {
    std::vector<float> out(n_tok * o);
    check(lmrs_debug_gemm_wide(device, out.data(), xq, xs, wq, ws, n, o, n_tok, q4 ? 1 : 0));
    return out;
}

// Unit-parity aid: the sort of forward_runs_sample's flat top-p rows on caller-supplied candidates, every row in one call of its launcher.  pairs: n_rows
// rows of ld {prob, index} entries, the first n0[r] of row r in index order -> a copy with those entries by descending prob, ties in index order
// (lmrs_op_sort_candidates)
struct ProbIndex { float prob; std::uint32_t index; };
inline std::vector<ProbIndex> op_sort_candidates(const std::vector<ProbIndex>& pairs, std::size_t ld, const std::vector<std::uint32_t>& n0, int device = 0) {
    std::vector<ProbIndex> sorted(pairs);
    check(lmrs_op_sort_candidates(device, pairs.data(), n0.size(), ld, n0.data(), sorted.data()));
    return sorted;
}

class Batch;

class Transformer {
public:
    TransformerArgs args{};

    // Transformer::new(&mmap) -> (Transformer, usize): `data` is the mapped LMRS file.
    static std::pair<Transformer, std::size_t> create(const std::uint8_t* data, std::size_t len, int device = 0) {
        Transformer t; std::size_t used = 0;
        check(lmrs_create(data, len, device, &t.ctx_, &used));
        t.args = *lmrs_get_args(t.ctx_);
        return {std::move(t), used};
    }
    Transformer(Transformer&& o) noexcept : args(o.args), ctx_(o.ctx_) { o.ctx_ = nullptr; }
    Transformer& operator=(Transformer&& o) noexcept { if (this != &o) { reset(); args = o.args; ctx_ = o.ctx_; o.ctx_ = nullptr; } return *this; }
    Transformer(const Transformer&) = delete;
    Transformer& operator=(const Transformer&) = delete;
    ~Transformer() { reset(); }

    // forward(&mut self, token, pos) -> &mut [f32]: vocab_size logits owned by the model, valid until the next call.
    float* forward(std::uint32_t token, std::uint32_t pos) { float* p = nullptr; check(lmrs_forward(ctx_, token, pos, &p)); return p; }
    // forward + Sampler::sample_argmax without moving the logits off the device.
    std::uint32_t forward_argmax(std::uint32_t token, std::uint32_t pos) { std::uint32_t n = 0; check(lmrs_forward_argmax(ctx_, token, pos, &n)); return n; }
    std::vector<float> get_embeddings(const std::vector<std::uint32_t>& tokens) const {
        std::vector<float> out(tokens.size() * args.dim);
        check(lmrs_get_embeddings(ctx_, tokens.data(), tokens.size(), out.data()));
        return out;
    }
    std::uint32_t fill_kv_cache(std::vector<float>& embeddings, std::uint32_t curr_pos) {
        std::uint32_t np = 0;
        check(lmrs_fill_kv_cache(ctx_, embeddings.data(), static_cast<std::uint32_t>(embeddings.size() / args.dim), curr_pos, &np));
        return np;
    }
    // forward + Sampler::sample with the logits staying in HBM (text.hpp: Sampler::forward_sample); `sampler`: a handle of lmrs_sampler_create.
    std::uint32_t forward_sample(std::uint32_t token, std::uint32_t pos, lmrs_sampler* sampler) { std::uint32_t n = 0; check(lmrs_forward_sample(ctx_, token, pos, sampler, &n)); return n; }
    // chat.rs:188-222 at temperature 0.
    std::vector<std::uint32_t> generate_greedy(const std::vector<std::uint32_t>& prompt, std::uint32_t n_new, std::uint32_t start_pos = 0, double* seconds = nullptr) {
        std::vector<std::uint32_t> out(n_new);
        check(lmrs_generate_greedy(ctx_, prompt.data(), prompt.size(), n_new, start_pos, out.data(), seconds));
        return out;
    }
    // Extension (no reference counterpart): forward(tokens[t], start_pos + t) for every t with the logits discarded - a prompt's K/V rows,
    // from token ids, batched on the device where the library says so (lmrs_tokens_path) -> start_pos + n.
    std::uint32_t prefill_tokens(const std::uint32_t* tokens, std::size_t n, std::uint32_t start_pos = 0) {
        std::uint32_t np = 0;
        check(lmrs_prefill_tokens(ctx_, tokens, n, start_pos, &np));
        return np;
    }
    std::uint32_t prefill_tokens(const std::vector<std::uint32_t>& tokens, std::uint32_t start_pos = 0) { return prefill_tokens(tokens.data(), tokens.size(), start_pos); }
    // Extensions (lmrs_verify_tokens / lmrs_generate_speculative): tokens[0] = the last confirmed token at start_pos, tokens[1..) = drafts -> the
    // argmax of every position and the number of accepted drafts, in one pass over the weights; generate_greedy's tokens by draft and verify
    struct Verified { std::vector<std::uint32_t> argmax; std::uint32_t n_accept = 0; };
    Verified verify_tokens(const std::vector<std::uint32_t>& tokens, std::uint32_t start_pos = 0) {
        Verified v; v.argmax.resize(tokens.size());
        check(lmrs_verify_tokens(ctx_, tokens.data(), tokens.size(), start_pos, v.argmax.data(), &v.n_accept));
        return v;
    }
    std::vector<std::uint32_t> generate_speculative(const std::vector<std::uint32_t>& prompt, std::uint32_t n_new, std::uint32_t start_pos = 0,
                                                    std::uint32_t max_draft = 7, std::uint32_t ngram_max = 3, std::uint32_t* stats4 = nullptr, double* seconds = nullptr) {
        std::vector<std::uint32_t> out(n_new);
        check(lmrs_generate_speculative(ctx_, prompt.data(), prompt.size(), n_new, start_pos, max_draft, ngram_max, out.data(), stats4, seconds));
        return out;
    }
    static std::vector<std::uint32_t> draft_lookup(const std::vector<std::uint32_t>& hist, std::uint32_t ngram_max, std::uint32_t max_draft) {
        std::vector<std::uint32_t> d(max_draft); std::uint32_t n = 0;
        check(lmrs_draft_lookup(hist.data(), hist.size(), ngram_max, max_draft, d.data(), &n));
        d.resize(n);
        return d;
    }
    bool tokens_path(std::size_t n) const { int b = 0; check(lmrs_tokens_path(ctx_, n, &b)); return b != 0; }
    // Extensions (no reference counterpart): one forward per token of `tokens` from position start_pos, in one call.
    // forward_tokens: n x vocab_size logits, row t = forward(tokens[t], start_pos + t).
    std::vector<float> forward_tokens(const std::vector<std::uint32_t>& tokens, std::uint32_t start_pos = 0) {
        std::vector<float> out(tokens.size() * static_cast<std::size_t>(args.vocab_size));
        check(lmrs_forward_tokens(ctx_, tokens.data(), tokens.size(), start_pos, out.data()));
        return out;
    }
    // score: log softmax(logits_t)[tokens[t+1]] for t < n-1, the argmax of every position, and the sum of the log-probabilities (double).
    struct Scores { std::vector<float> logprobs; std::vector<std::uint32_t> argmax; double sum_logprob = 0.0; };
    Scores score(const std::vector<std::uint32_t>& tokens, std::uint32_t start_pos = 0) {
        Scores s;
        s.logprobs.resize(tokens.empty() ? 0 : tokens.size() - 1); s.argmax.resize(tokens.size());
        check(lmrs_score_tokens(ctx_, tokens.data(), tokens.size(), start_pos, s.logprobs.data(), s.argmax.data(), &s.sum_logprob));
        return s;
    }
    // score_topk: score with the k first next-token candidates of every position (1 <= k <= 256, k <= vocab_size), selected on the device: the
    // larger logit first, equal logits by ascending index, NaNs last (a NaN at index 0 first: rank 0 is argmax[t]).  topk_idx / topk_logprob:
    // n x k, the log-probabilities with logprobs' maximum and sum; target_rank[t]: the candidates that precede tokens[t+1], whatever k is.
    struct ScoreTopk : Scores { std::uint32_t k = 0; std::vector<std::uint32_t> topk_idx; std::vector<float> topk_logprob; std::vector<std::uint32_t> target_rank; };
    ScoreTopk score_topk(const std::vector<std::uint32_t>& tokens, std::uint32_t k, std::uint32_t start_pos = 0) {
        ScoreTopk s;
        const std::size_t n = tokens.size();
        s.k = k; s.logprobs.resize(n ? n - 1 : 0); s.argmax.resize(n); s.target_rank.resize(n ? n - 1 : 0);
        s.topk_idx.resize(n * k); s.topk_logprob.resize(n * k);
        check(lmrs_score_tokens_topk(ctx_, tokens.data(), n, start_pos, k, s.logprobs.data(), s.argmax.data(), &s.sum_logprob, s.topk_idx.data(),
                                     s.topk_logprob.data(), s.target_rank.data()));
        return s;
    }
    // forward + the selection of the k first candidates on the device -> (indices, their raw logits) in score_topk's order; 2k words cross to the host.
    std::pair<std::vector<std::uint32_t>, std::vector<float>> forward_topk(std::uint32_t token, std::uint32_t pos, std::uint32_t k) {
        std::vector<std::uint32_t> idx(k); std::vector<float> val(k);
        check(lmrs_forward_topk(ctx_, token, pos, k, idx.data(), val.data()));
        return {std::move(idx), std::move(val)};
    }

private:
    friend class Batch;
    Transformer() = default;
    void reset() { if (ctx_) { lmrs_destroy(ctx_); ctx_ = nullptr; } }
    lmrs_ctx* ctx_ = nullptr;
};

// Extension (lmrs_batch_*): n_slots (1 .. 16) K/V caches beside the transformer's own, stepped together - one pass over the weights serves one
// token of up to 16 different sequences.  Every result is bit for bit forward's on a transformer that holds only that sequence; the transformer's
// own cache is untouched.  Destroy the batch before its transformer.
class Batch {
public:
    static constexpr std::uint32_t CTX = LMRS_BATCH_CTX;           // fork's source: the transformer's own cache
    // wide: up to 64 slots, and forward / generate_greedy / forward_runs / forward_runs_sample take up to 64 rows or runs a call (lmrs_batch_create_wide)
    Batch(Transformer& t, std::uint32_t n_slots, bool wide = false) : vocab_size_(t.args.vocab_size) {
        check(wide ? lmrs_batch_create_wide(t.ctx_, n_slots, &b_) : lmrs_batch_create(t.ctx_, n_slots, &b_));
    }
    // a PAGED batch (wide): the slots draw pages of page_len positions (64, 128, 256, 512 or 1024) from one pool of n_pages pages; fork shares whole pages,
    // a write un-shares the page it touches, release gives pages back.  Without release every result is a wide batch's, bit for bit  (lmrs_batch_create_paged)
    Batch(Transformer& t, std::uint32_t n_slots, std::uint32_t page_len, std::uint32_t n_pages) : vocab_size_(t.args.vocab_size) {
        check(lmrs_batch_create_paged(t.ctx_, n_slots, page_len, n_pages, &b_));
    }
    struct Pages { std::uint32_t page_len, n_pages, n_free; };
    Pages pages() const { Pages p{}; check(lmrs_batch_pages(b_, &p.page_len, &p.n_pages, &p.n_free)); return p; }                  // (lmrs_batch_pages)
    struct SlotPages { std::uint32_t held, shared; };
    SlotPages slot_pages(std::uint32_t slot) const { SlotPages p{}; check(lmrs_batch_slot_pages(b_, slot, &p.held, &p.shared)); return p; }   // (lmrs_batch_slot_pages)
    // keep positions [0, n_pos) of a slot (0 empties it): the pages behind them return to the pool once nobody holds them  (lmrs_batch_release)
    void release(std::uint32_t slot, std::uint32_t n_pos = 0) { check(lmrs_batch_release(b_, slot, n_pos)); }
    // how prefill / prefill_embeddings would run n rows at start_pos: passes of at most 512 rows, and how many of them take block attention (64-query
    // blocks; the others one workgroup per (head, row)).  Host arithmetic only, any batch  (lmrs_batch_prefill_form)
    struct PrefillForm { std::uint32_t n_chunks, n_block; };
    PrefillForm prefill_form(std::size_t n, std::uint32_t start_pos = 0) const { PrefillForm f{}; check(lmrs_batch_prefill_form(b_, n, start_pos, &f.n_chunks, &f.n_block)); return f; }
    // test / A-B aid: every prompt chunk of this PAGED batch takes the table pass from now on (false: the library's rule)  (lmrs_batch_debug_prefill_table)
    void debug_prefill_table(bool force = true) { check(lmrs_batch_debug_prefill_table(b_, force ? 1 : 0)); }
    // Allowed-token masks, state of a slot: bits = mask_words() words per slot, bit (t & 31) of word (t >> 5) set = token t allowed.  While a slot has a
    // mask every output row of it in any call here - logits, argmax, top-k, sampled token - comes from the row's logits with the disallowed entries -inf;
    // the mask stays until it is replaced or cleared  (lmrs_batch_set_masks / lmrs_batch_clear_masks / lmrs_batch_mask_info)
    std::size_t mask_words() const { return (vocab_size_ + 31) / 32; }
    void set_masks(const std::vector<std::uint32_t>& slot, const std::vector<std::uint32_t>& bits) {
        if (bits.size() != slot.size() * mask_words()) throw Panic("Batch::set_masks: bits must hold mask_words() words per slot");
        check(lmrs_batch_set_masks(b_, static_cast<std::uint32_t>(slot.size()), slot.data(), bits.data()));
    }
    void clear_masks() { check(lmrs_batch_clear_masks(b_, 0, nullptr)); }                                      // every slot
    void clear_masks(const std::vector<std::uint32_t>& slot) {
        if (!slot.empty()) check(lmrs_batch_clear_masks(b_, static_cast<std::uint32_t>(slot.size()), slot.data()));
    }
    std::uint32_t mask_info(std::uint32_t slot) const { std::uint32_t n = 0; check(lmrs_batch_mask_info(b_, slot, &n)); return n; }   // the tokens allowed; 0: no mask
    // Token automata: a DFA over tokens - class_of[vocab_size] below n_classes, next[n_states * n_classes] a state or STATE_DEAD, a final flag per state (empty:
    // none) - whose tables and per-state masks stay on the device.  A slot attached to one has the mask of its current state in every call here; generate /
    // generate_topp move the state with every token they choose and end a row that reaches a final state with FINISH_FINAL; advance moves it by hand
    // (lmrs_batch_automaton_create / _destroy, lmrs_batch_attach_automaton, lmrs_batch_automaton_state / _advance)
    static constexpr std::uint32_t STATE_DEAD = LMRS_STATE_DEAD, FINISH_FINAL = LMRS_FINISH_FINAL;
    lmrs_automaton* automaton(std::uint32_t n_states, std::uint32_t n_classes, const std::vector<std::uint16_t>& class_of, const std::vector<std::uint32_t>& next,
                              const std::vector<std::uint8_t>& final_states = {}) {
        if (class_of.size() != vocab_size_ || next.size() != static_cast<std::size_t>(n_states) * n_classes || (!final_states.empty() && final_states.size() != n_states))
            throw Panic("Batch::automaton: class_of holds vocab_size entries, next n_states * n_classes, final_states none or n_states");
        lmrs_automaton* a = nullptr;
        check(lmrs_batch_automaton_create(b_, n_states, n_classes, class_of.data(), next.data(), final_states.empty() ? nullptr : final_states.data(), &a));
        return a;
    }
    void drop_automaton(lmrs_automaton* a) { check(lmrs_batch_automaton_destroy(b_, a)); }                     // refused while a slot is attached to it
    void attach(const std::vector<std::uint32_t>& slot, const std::vector<lmrs_automaton*>& a, const std::vector<std::uint32_t>& state) {   // a[i] null: detach
        if (a.size() != slot.size() || state.size() != slot.size()) throw Panic("Batch::attach: one automaton and one state per slot");
        check(lmrs_batch_attach_automaton(b_, static_cast<std::uint32_t>(slot.size()), slot.data(), a.data(), state.data()));
    }
    struct AutomatonState { bool attached; std::uint32_t state, n_allowed; bool is_final; };
    AutomatonState automaton_state(std::uint32_t slot) const {
        std::uint32_t q = 0, n = 0; int f = 0;
        check(lmrs_batch_automaton_state(b_, slot, &q, &n, &f));
        return AutomatonState{q != STATE_DEAD, q, n, f != 0};
    }
    void advance(std::uint32_t slot, const std::vector<std::uint32_t>& tokens) { check(lmrs_batch_automaton_advance(b_, slot, tokens.data(), tokens.size())); }
    // Repetition / presence / frequency penalties, state of a slot, over the token record the batch keeps on the device from the first of these calls on
    // (include/lmrs_hip.h: the rule): tokens the slot has seen anywhere are divided / multiplied by `repetition`, tokens seen at positions >= out_from lose
    // frequency * count + presence, in front of the slot's mask and of every sink  (lmrs_batch_set_penalties / _clear_penalties / _penalty_info)
    struct Penalty { float repetition = 1.0f, presence = 0.0f, frequency = 0.0f; std::uint32_t out_from = 0; bool active = false; };
    static constexpr std::uint32_t TOKEN_NONE = LMRS_TOKEN_NONE;   // the record's word for an unknown token or an embedding row
    void set_penalties(const std::vector<std::uint32_t>& slot, const std::vector<Penalty>& p) {
        if (p.size() != slot.size()) throw Panic("Batch::set_penalties: one Penalty per slot");
        std::vector<float> rep, pres, freq; std::vector<std::uint32_t> from;
        for (const Penalty& x : p) { rep.push_back(x.repetition); pres.push_back(x.presence); freq.push_back(x.frequency); from.push_back(x.out_from); }
        check(lmrs_batch_set_penalties(b_, static_cast<std::uint32_t>(slot.size()), slot.data(), rep.data(), pres.data(), freq.data(), from.data()));
    }
    void clear_penalties() { check(lmrs_batch_clear_penalties(b_, 0, nullptr)); }                              // every slot
    void clear_penalties(const std::vector<std::uint32_t>& slot) {
        if (!slot.empty()) check(lmrs_batch_clear_penalties(b_, static_cast<std::uint32_t>(slot.size()), slot.data()));
    }
    Penalty penalty_info(std::uint32_t slot) const {
        Penalty p; int active = 0;
        check(lmrs_batch_penalty_info(b_, slot, &p.repetition, &p.presence, &p.frequency, &p.out_from, &active));
        p.active = active != 0;
        return p;
    }
    // the record of `slot` from start_pos on: written by the caller (positions filled before the record existed; no tokens: only switches it on), read back
    void set_history(std::uint32_t slot, const std::vector<std::uint32_t>& tokens = {}, std::uint32_t start_pos = 0) {
        check(lmrs_batch_set_history(b_, slot, start_pos, tokens.empty() ? nullptr : tokens.data(), tokens.size()));
    }
    std::vector<std::uint32_t> history(std::uint32_t slot, std::size_t n, std::uint32_t start_pos = 0) {
        std::vector<std::uint32_t> out(n);
        check(lmrs_batch_history(b_, slot, start_pos, n, n ? out.data() : nullptr));
        return out;
    }
    // Candidate filters, state of a slot (include/lmrs_hip.h: the rule): every logit outside the row's first top_k candidates (0: off) and every logit more
    // than min_gap below the largest (+inf: off; min_p_gap turns a min_p into it) reads -inf, behind the penalties and the mask and in front of every sink
    // but generate_greedy's  (lmrs_batch_set_filters / _clear_filters / _filter_info; filter_rows: the kernel alone, lmrs_op_filter_rows)
    struct Filter { std::uint32_t top_k = 0; float min_gap = HUGE_VALF; bool active = false; };
    static float min_p_gap(double min_p, double temperature) { return min_p > 0.0 ? static_cast<float>(-temperature * std::log(min_p) + 0.0) : HUGE_VALF; }
    void set_filters(const std::vector<std::uint32_t>& slot, const std::vector<Filter>& f) {
        if (f.size() != slot.size()) throw Panic("Batch::set_filters: one Filter per slot");
        std::vector<std::uint32_t> k; std::vector<float> gap;
        for (const Filter& x : f) { k.push_back(x.top_k); gap.push_back(x.min_gap); }
        check(lmrs_batch_set_filters(b_, static_cast<std::uint32_t>(slot.size()), slot.data(), k.data(), gap.data()));
    }
    void clear_filters() { check(lmrs_batch_clear_filters(b_, 0, nullptr)); }                                  // every slot
    void clear_filters(const std::vector<std::uint32_t>& slot) {
        if (!slot.empty()) check(lmrs_batch_clear_filters(b_, static_cast<std::uint32_t>(slot.size()), slot.data()));
    }
    Filter filter_info(std::uint32_t slot) const {
        Filter f; int active = 0;
        check(lmrs_batch_filter_info(b_, slot, &f.top_k, &f.min_gap, &active));
        f.active = active != 0;
        return f;
    }
    static void filter_rows(int device, float* rows, std::size_t n_rows, std::size_t n, std::size_t ld, const std::vector<Filter>& f) {
        if (f.size() != n_rows) throw Panic("Batch::filter_rows: one Filter per row");
        std::vector<std::uint32_t> k; std::vector<float> gap;
        for (const Filter& x : f) { k.push_back(x.top_k); gap.push_back(x.min_gap); }
        check(lmrs_op_filter_rows(device, rows, n_rows, n, ld, k.data(), gap.data()));
    }
    // the most rows (forward, generate_greedy) and runs (forward_runs) a call takes: 16, or 64 for a wide batch  (lmrs_batch_width)
    std::uint32_t width() const { std::uint32_t w = 0; check(lmrs_batch_width(b_, &w)); return w; }
    Batch(const Batch&) = delete;
    Batch& operator=(const Batch&) = delete;
    ~Batch() { if (b_) lmrs_batch_destroy(b_); }
    void prefill(std::uint32_t slot, const std::vector<std::uint32_t>& tokens, std::uint32_t start_pos = 0) {
        check(lmrs_batch_prefill(b_, slot, tokens.data(), tokens.size(), start_pos));
    }
    // ONE fill_kv_cache call (transformer.rs:672-684) into slot's cache: n = embeddings.size() / dim rows, taken as given, at start_pos ..; residual
    // (optional): what the reference leaves in its mutated argument - without it nothing is downloaded  (lmrs_batch_prefill_embeddings)
    void prefill_embeddings(std::uint32_t slot, const std::vector<float>& embeddings, std::uint32_t n, std::uint32_t start_pos = 0, std::vector<float>* residual = nullptr) {
        if (residual) residual->resize(embeddings.size());
        check(lmrs_batch_prefill_embeddings(b_, slot, embeddings.data(), n, start_pos, residual ? residual->data() : nullptr));
    }
    void fork(std::uint32_t src_slot, std::uint32_t dst_slot, std::uint32_t n_pos) { check(lmrs_batch_fork(b_, src_slot, dst_slot, n_pos)); }
    // row i = forward(tokens[i], pos[i]) on slot[i] -> the argmax of every row; logits (optional): n x vocab_size
    std::vector<std::uint32_t> forward(const std::vector<std::uint32_t>& slot, const std::vector<std::uint32_t>& tokens, const std::vector<std::uint32_t>& pos,
                                       std::vector<float>* logits = nullptr) {
        if (slot.size() != tokens.size() || slot.size() != pos.size()) throw Panic("Batch::forward: one slot, token and position per row");
        std::vector<std::uint32_t> argmax(slot.size());
        if (logits) logits->resize(slot.size() * vocab_size_);
        check(lmrs_batch_forward(b_, static_cast<std::uint32_t>(slot.size()), slot.data(), tokens.data(), pos.data(), argmax.data(), logits ? logits->data() : nullptr));
        return argmax;
    }
    // forward with a sampler per row, sampled on the device: row i = forward(tokens[i], pos[i]) on slot[i] followed by Sampler::sample with samplers[i]
    // (Sampler::handle(), text.hpp) -> next[i], bit for bit Transformer::forward_sample's token on a transformer that holds only that sequence.  Rows may
    // mix samplers; a top-p sampler in at most one row of a call  (lmrs_batch_forward_sample)
    std::vector<std::uint32_t> forward_sample(const std::vector<std::uint32_t>& slot, const std::vector<std::uint32_t>& tokens, const std::vector<std::uint32_t>& pos,
                                              const std::vector<lmrs_sampler*>& samplers) {
        if (slot.size() != tokens.size() || slot.size() != pos.size() || slot.size() != samplers.size()) throw Panic("Batch::forward_sample: one slot, token, position and sampler per row");
        std::vector<std::uint32_t> next(slot.size());
        check(lmrs_batch_forward_sample(b_, static_cast<std::uint32_t>(slot.size()), slot.data(), tokens.data(), pos.data(), samplers.data(), next.data()));
        return next;
    }
    // n_new greedy steps of every row on the device: out[i * n_new + j]
    std::vector<std::uint32_t> generate_greedy(const std::vector<std::uint32_t>& slot, const std::vector<std::uint32_t>& tokens, const std::vector<std::uint32_t>& pos,
                                               std::uint32_t n_new, double* seconds = nullptr) {
        if (slot.size() != tokens.size() || slot.size() != pos.size()) throw Panic("Batch::generate_greedy: one slot, token and position per row");
        std::vector<std::uint32_t> out(slot.size() * n_new);
        check(lmrs_batch_generate_greedy(b_, static_cast<std::uint32_t>(slot.size()), slot.data(), tokens.data(), pos.data(), n_new, out.data(), seconds));
        return out;
    }
    // The device loop whose rows end one by one: row i feeds tokens[i] at pos[i] of slot[i] and goes on with what it chose - Sampler::sample with samplers[i]
    // (Sampler::handle(), text.hpp; argmax and sample_mult samplers, top-p is refused), the argmax for a null entry or an empty `samplers` - until it chooses a
    // token of stop[i] (FINISH_STOP: the token is reported, never fed) or has produced max_new[i] tokens (FINISH_BUDGET).  stop: empty, or one set (at most
    // STOP_MAX tokens) per row.  check_every: passes between two looks at the rows' state; no result depends on it  (lmrs_batch_generate)
    static constexpr std::uint32_t STOP_MAX = LMRS_STOP_MAX, FINISH_BUDGET = LMRS_FINISH_BUDGET, FINISH_STOP = LMRS_FINISH_STOP,
                                   FINISH_NO_CANDIDATE = LMRS_FINISH_NO_CANDIDATE;
    struct Generated {
        std::vector<std::vector<std::uint32_t>> tokens;      // row i's outputs, n_out[i] of them
        std::vector<std::vector<float>> logprobs;            // with logprobs: log softmax of the row each token was chosen from, at that token
        std::vector<std::uint32_t> finish;
        std::uint64_t passes = 0, row_passes = 0; double seconds = 0.0;
    };
    Generated generate(const std::vector<std::uint32_t>& slot, const std::vector<std::uint32_t>& tokens, const std::vector<std::uint32_t>& pos,
                       const std::vector<std::uint32_t>& max_new, const std::vector<std::vector<std::uint32_t>>& stop = {},
                       const std::vector<lmrs_sampler*>& samplers = {}, std::uint32_t check_every = 4, bool logprobs = false) {
        return generate_by(false, slot, tokens, pos, max_new, stop, samplers, check_every, logprobs);
    }
    // generate with top-p samplers admitted, each in one row only: their candidate vectors live on the device for the length of the call and are back in
    // the samplers when it returns.  A row whose step finds no candidate above the cutoff ends with FINISH_NO_CANDIDATE and reports no token for that
    // step  (lmrs_batch_generate_topp)
    Generated generate_topp(const std::vector<std::uint32_t>& slot, const std::vector<std::uint32_t>& tokens, const std::vector<std::uint32_t>& pos,
                            const std::vector<std::uint32_t>& max_new, const std::vector<std::vector<std::uint32_t>>& stop = {},
                            const std::vector<lmrs_sampler*>& samplers = {}, std::uint32_t check_every = 4, bool logprobs = false) {
        return generate_by(true, slot, tokens, pos, max_new, stop, samplers, check_every, logprobs);
    }
    Generated generate_by(bool topp, const std::vector<std::uint32_t>& slot, const std::vector<std::uint32_t>& tokens, const std::vector<std::uint32_t>& pos,
                          const std::vector<std::uint32_t>& max_new, const std::vector<std::vector<std::uint32_t>>& stop,
                          const std::vector<lmrs_sampler*>& samplers, std::uint32_t check_every, bool logprobs) {
        const std::size_t n = slot.size();
        if (tokens.size() != n || pos.size() != n || max_new.size() != n) throw Panic("Batch::generate: one slot, token, position and budget per row");
        if (!stop.empty() && stop.size() != n) throw Panic("Batch::generate: stop is empty or holds one set per row");
        if (!samplers.empty() && samplers.size() != n) throw Panic("Batch::generate: samplers is empty or holds one entry per row");
        std::vector<std::uint32_t> n_stop, packed;
        for (const auto& s : stop) { n_stop.push_back(static_cast<std::uint32_t>(s.size())); packed.insert(packed.end(), s.begin(), s.end()); }
        std::uint32_t M = 1;
        for (std::uint32_t m : max_new) M = m > M ? m : M;
        std::vector<std::uint32_t> out(n * M), n_out(n), fin(n);
        std::vector<float> lp(logprobs ? n * M : 0);
        std::uint64_t stats[2] = {0, 0};
        Generated g;
        const std::uint32_t* ns = stop.empty() ? nullptr : n_stop.data(); const std::uint32_t* st = packed.empty() ? nullptr : packed.data();
        lmrs_sampler* const* sm = samplers.empty() ? nullptr : samplers.data(); float* lps = logprobs ? lp.data() : nullptr;
        const std::uint32_t rows = static_cast<std::uint32_t>(n);
        check(topp ? lmrs_batch_generate_topp(b_, rows, slot.data(), tokens.data(), pos.data(), max_new.data(), ns, st, sm, check_every, out.data(), lps, n_out.data(),
                                              fin.data(), stats, &g.seconds)
                   : lmrs_batch_generate(b_, rows, slot.data(), tokens.data(), pos.data(), max_new.data(), ns, st, sm, check_every, out.data(), lps, n_out.data(),
                                         fin.data(), stats, &g.seconds));
        for (std::size_t i = 0; i < n; ++i) {
            g.tokens.emplace_back(out.begin() + i * M, out.begin() + i * M + n_out[i]);
            if (logprobs) g.logprobs.emplace_back(lp.begin() + i * M, lp.begin() + i * M + n_out[i]);
        }
        g.finish = fin; g.passes = stats[0]; g.row_passes = stats[1];
        return g;
    }
    // One pass over runs of consecutive tokens, one run per slot (a prompt chunk, a draft to verify, one decode row; at most 512 tokens in all): outputs for
    // the LAST n_out rows of every run, packed in run order - argmax always, logits (x vocab_size) and the k first candidates with their log-probabilities
    // (x k, as lmrs_score_tokens_topk defines them) when asked for  (lmrs_batch_forward_runs)
    // A run with `embeddings` (rows x dim floats, `tokens` empty) feeds those rows instead of token ids, each as fill_kv_cache(&row, 1, its position)
    // takes it; the call then goes through lmrs_batch_forward_runs_embed
    struct Run { std::uint32_t slot, start_pos; std::vector<std::uint32_t> tokens; std::uint32_t n_out; std::vector<float> embeddings = {}; std::uint32_t n_embed = 0; };
    struct RunsOut { std::vector<std::uint32_t> argmax; std::vector<float> logits; std::vector<std::uint32_t> topk_idx; std::vector<float> topk_logprob; };
    RunsOut forward_runs(const std::vector<Run>& runs, std::uint32_t k = 0, bool logits = false) {
        std::vector<std::uint32_t> slot, start, len, n_out, tokens, kind;
        std::vector<float> embeddings;
        std::size_t rows = 0;
        bool embed = false;
        for (const Run& r : runs) {
            const bool e = r.n_embed > 0;
            if (e && !r.tokens.empty()) throw Panic("Batch::forward_runs: a run holds tokens or embeddings, not both");
            slot.push_back(r.slot); start.push_back(r.start_pos); len.push_back(e ? r.n_embed : static_cast<std::uint32_t>(r.tokens.size())); n_out.push_back(r.n_out);
            kind.push_back(e ? 1u : 0u);
            tokens.insert(tokens.end(), r.tokens.begin(), r.tokens.end());
            embeddings.insert(embeddings.end(), r.embeddings.begin(), r.embeddings.end());
            rows += r.n_out;
            embed = embed || e;
        }
        RunsOut o;
        o.argmax.resize(rows); o.topk_idx.resize(rows * k); o.topk_logprob.resize(rows * k);
        if (logits) o.logits.resize(rows * vocab_size_);
        if (embed) {
            check(lmrs_batch_forward_runs_embed(b_, static_cast<std::uint32_t>(runs.size()), slot.data(), start.data(), len.data(), n_out.data(), kind.data(),
                                                tokens.empty() ? nullptr : tokens.data(), embeddings.data(), rows ? o.argmax.data() : nullptr,
                                                logits ? o.logits.data() : nullptr, k, k ? o.topk_idx.data() : nullptr, k ? o.topk_logprob.data() : nullptr));
            return o;
        }
        check(lmrs_batch_forward_runs(b_, static_cast<std::uint32_t>(runs.size()), slot.data(), start.data(), len.data(), n_out.data(), tokens.data(),
                                      rows ? o.argmax.data() : nullptr, logits ? o.logits.data() : nullptr, k, k ? o.topk_idx.data() : nullptr,
                                      k ? o.topk_logprob.data() : nullptr));
        return o;
    }
    // forward_runs with a sampler per run, sampled on the device: the LAST row of every run whose sampler (Sampler::handle(), text.hpp) is not null goes
    // through Sampler::sample with it -> next[i], bit for bit Transformer::forward_sample's token after the run's tokens on a transformer that holds only
    // that sequence; a null sampler leaves the run's K/V rows only and next[i] = 0.  Up to width() runs; runs may mix samplers, a top-p sampler in at most
    // one run of a call  (lmrs_batch_forward_runs_sample)
    // (a run with `embeddings`, as in Run: the call goes through lmrs_batch_forward_runs_embed_sample)
    struct SampledRun { std::uint32_t slot, start_pos; std::vector<std::uint32_t> tokens; lmrs_sampler* sampler; std::vector<float> embeddings = {}; std::uint32_t n_embed = 0; };
    std::vector<std::uint32_t> forward_runs_sample(const std::vector<SampledRun>& runs) {
        std::vector<std::uint32_t> slot, start, len, tokens, kind, next(runs.size());
        std::vector<float> embeddings;
        std::vector<lmrs_sampler*> samplers;
        bool embed = false;
        for (const SampledRun& r : runs) {
            const bool e = r.n_embed > 0;
            if (e && !r.tokens.empty()) throw Panic("Batch::forward_runs_sample: a run holds tokens or embeddings, not both");
            slot.push_back(r.slot); start.push_back(r.start_pos); len.push_back(e ? r.n_embed : static_cast<std::uint32_t>(r.tokens.size())); samplers.push_back(r.sampler);
            kind.push_back(e ? 1u : 0u);
            tokens.insert(tokens.end(), r.tokens.begin(), r.tokens.end());
            embeddings.insert(embeddings.end(), r.embeddings.begin(), r.embeddings.end());
            embed = embed || e;
        }
        if (embed) {
            check(lmrs_batch_forward_runs_embed_sample(b_, static_cast<std::uint32_t>(runs.size()), slot.data(), start.data(), len.data(), kind.data(),
                                                       tokens.empty() ? nullptr : tokens.data(), embeddings.data(), samplers.data(), next.data()));
            return next;
        }
        check(lmrs_batch_forward_runs_sample(b_, static_cast<std::uint32_t>(runs.size()), slot.data(), start.data(), len.data(), tokens.data(), samplers.data(),
                                             next.data()));
        return next;
    }
    void debug_kv(std::uint32_t slot, int which, std::uint32_t layer, std::uint32_t pos, float* out) { check(lmrs_batch_debug_kv(b_, slot, which, layer, pos, out)); }

private:
    lmrs_batch* b_ = nullptr;
    std::size_t vocab_size_ = 0;
};

}  // namespace lmrs_host
