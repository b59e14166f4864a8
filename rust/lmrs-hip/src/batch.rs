//! `Batch`: up to 16 sequences a step (64 with `Batch::new_wide`) over the weights of one `Transformer` (extension, no reference counterpart; include/lmrs_hip.h,
//! `lmrs_batch_*`).  Each slot is a K/V cache of its own; every result is bit for bit what `Transformer::forward` gives on a context that holds
//! only that sequence.  The borrow keeps the transformer alive and un-aliased while the batch exists.
use std::os::raw::c_int;
use std::ptr;

use crate::ffi::{self, check, LmrsBatch, LmrsSampler};
use crate::sampler::Sampler;
use crate::transformer::Transformer;

// The sampled step (include/lmrs_hip.h, lmrs_batch_forward_sample): declared beside its only caller; the batch block of ffi.rs holds the greedy entry
// points (tests/test_batch_sample_host.py compares this declaration with the header).
extern "C" {
    pub fn lmrs_batch_forward_sample(b: *mut LmrsBatch, n: u32, slot: *const u32, tokens: *const u32, pos: *const u32,
                                     samplers: *const *mut LmrsSampler, next: *mut u32) -> c_int;
    // the wide batch (lmrs_batch_create_wide): declared here for the same reason (tests/test_batch_wide_host.py compares them with the header)
    pub fn lmrs_batch_create_wide(ctx: *mut ffi::LmrsCtx, n_slots: u32, out: *mut *mut LmrsBatch) -> c_int;
    pub fn lmrs_batch_width(b: *const LmrsBatch, width: *mut u32) -> c_int;
    // the sampled ragged pass: declared here as the sampled step is (tests/test_batch_runs_sample_host.py compares it with the header)
    pub fn lmrs_batch_forward_runs_sample(b: *mut LmrsBatch, n_runs: u32, slot: *const u32, start_pos: *const u32, run_len: *const u32,
                                          tokens: *const u32, samplers: *const *mut LmrsSampler, next: *mut u32) -> c_int;
    // embedding rows in a slot and in the ragged passes: declared here as the sampled calls are (tests/test_batch_embed_host.py compares them with the header)
    pub fn lmrs_batch_prefill_embeddings(b: *mut LmrsBatch, slot: u32, embeddings: *const f32, n: u32, start_pos: u32, residual: *mut f32) -> c_int;
    pub fn lmrs_batch_forward_runs_embed(b: *mut LmrsBatch, n_runs: u32, slot: *const u32, start_pos: *const u32, run_len: *const u32, n_out: *const u32,
                                         run_kind: *const u32, tokens: *const u32, embeddings: *const f32, argmax: *mut u32, logits: *mut f32,
                                         k: u32, topk_idx: *mut u32, topk_logprob: *mut f32) -> c_int;
    pub fn lmrs_batch_forward_runs_embed_sample(b: *mut LmrsBatch, n_runs: u32, slot: *const u32, start_pos: *const u32, run_len: *const u32,
                                                run_kind: *const u32, tokens: *const u32, embeddings: *const f32,
                                                samplers: *const *mut LmrsSampler, next: *mut u32) -> c_int;
    // paged K/V: declared here as the wide batch is (tests/test_batch_paged_host.py compares them with the header)
    pub fn lmrs_batch_create_paged(ctx: *mut ffi::LmrsCtx, n_slots: u32, page_len: u32, n_pages: u32, out: *mut *mut LmrsBatch) -> c_int;
    pub fn lmrs_batch_pages(b: *const LmrsBatch, page_len: *mut u32, n_pages: *mut u32, n_free: *mut u32) -> c_int;
    pub fn lmrs_batch_slot_pages(b: *const LmrsBatch, slot: u32, n_held: *mut u32, n_shared: *mut u32) -> c_int;
    pub fn lmrs_batch_release(b: *mut LmrsBatch, slot: u32, n_pos: u32) -> c_int;
    pub fn lmrs_batch_prefill_form(b: *const LmrsBatch, n: usize, start_pos: u32, n_chunks: *mut u32, n_block: *mut u32) -> c_int;
    pub fn lmrs_batch_debug_prefill_table(b: *mut LmrsBatch, force: c_int) -> c_int;
    // the token record per slot and the penalties over it: declared here as the paged calls are (tests/test_batch_penalty_host.py compares them with the
    // header; the batch block of ffi.rs keeps its seven entry points, tests/test_batch.py)
    pub fn lmrs_batch_set_history(b: *mut LmrsBatch, slot: u32, start_pos: u32, tokens: *const u32, n: usize) -> c_int;
    pub fn lmrs_batch_history(b: *mut LmrsBatch, slot: u32, start_pos: u32, n: usize, out: *mut u32) -> c_int;
    pub fn lmrs_batch_set_penalties(b: *mut LmrsBatch, n: u32, slot: *const u32, repetition: *const f32, presence: *const f32,
                                    frequency: *const f32, out_from: *const u32) -> c_int;
    pub fn lmrs_batch_clear_penalties(b: *mut LmrsBatch, n: u32, slot: *const u32) -> c_int;
    pub fn lmrs_batch_penalty_info(b: *const LmrsBatch, slot: u32, repetition: *mut f32, presence: *mut f32, frequency: *mut f32,
                                   out_from: *mut u32, active: *mut c_int) -> c_int;
    // the device loop whose rows end one by one: declared here as the penalty calls are (tests/test_batch_generate_host.py compares it with the header)
    pub fn lmrs_batch_generate(b: *mut LmrsBatch, n: u32, slot: *const u32, tokens: *const u32, pos: *const u32, max_new: *const u32,
                               n_stop: *const u32, stop_tokens: *const u32, samplers: *const *mut LmrsSampler, check_every: u32,
                               out_tokens: *mut u32, out_logprobs: *mut f32, n_out: *mut u32, finish: *mut u32, stats2: *mut u64,
                               seconds: *mut f64) -> c_int;
    pub fn lmrs_batch_generate_topp(b: *mut LmrsBatch, n: u32, slot: *const u32, tokens: *const u32, pos: *const u32, max_new: *const u32,
                                    n_stop: *const u32, stop_tokens: *const u32, samplers: *const *mut LmrsSampler, check_every: u32,
                                    out_tokens: *mut u32, out_logprobs: *mut f32, n_out: *mut u32, finish: *mut u32, stats2: *mut u64,
                                    seconds: *mut f64) -> c_int;
    // candidate filters per slot, and the kernel alone on caller rows: declared here as the penalty calls are (tests/test_batch_filter_host.py compares them
    // with the header)
    pub fn lmrs_batch_set_filters(b: *mut LmrsBatch, n: u32, slot: *const u32, top_k: *const u32, min_gap: *const f32) -> c_int;
    pub fn lmrs_batch_clear_filters(b: *mut LmrsBatch, n: u32, slot: *const u32) -> c_int;
    pub fn lmrs_batch_filter_info(b: *const LmrsBatch, slot: u32, top_k: *mut u32, min_gap: *mut f32, active: *mut c_int) -> c_int;
    pub fn lmrs_op_filter_rows(device: c_int, rows: *mut f32, n_rows: usize, n: usize, ld: usize, top_k: *const u32, min_gap: *const f32) -> c_int;
}

/// A slot's candidate filters (`Batch::set_filters`): every logit outside the row's first `top_k` candidates (0: off) and every logit more than `min_gap`
/// below the largest (`f32::INFINITY`: off) reads `-inf` in front of every sink (include/lmrs_hip.h: the rule).
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct Filter {
    pub top_k: u32,
    pub min_gap: f32,
}

/// The `min_gap` that keeps the tokens whose probability at `temperature` is at least `min_p` times the largest: `-temperature * ln(min_p)`, formed in
/// f64 and rounded once.
pub fn min_p_gap(min_p: f64, temperature: f64) -> f32 {
    if min_p > 0.0 { (-temperature * min_p.ln() + 0.0) as f32 } else { f32::INFINITY }
}

/// The filter kernel alone over `n_rows` rows of `n` logits at stride `ld`, in place (`lmrs_op_filter_rows`).
pub fn filter_rows(device: i32, rows: &mut [f32], n_rows: usize, n: usize, ld: usize, filters: &[Filter]) {
    assert!(filters.len() == n_rows && rows.len() >= n_rows * ld, "one Filter per row, n_rows * ld floats");
    let k: Vec<u32> = filters.iter().map(|f| f.top_k).collect();
    let gap: Vec<f32> = filters.iter().map(|f| f.min_gap).collect();
    check(unsafe { lmrs_op_filter_rows(device as c_int, rows.as_mut_ptr(), n_rows, n, ld, k.as_ptr(), gap.as_ptr()) });
}

/// The most stop tokens a row of `Batch::generate` takes (`LMRS_STOP_MAX`).
pub const STOP_MAX: usize = 16;
/// `Batch::generate`'s finish codes (`LMRS_FINISH_BUDGET`, `LMRS_FINISH_STOP`).
pub const FINISH_BUDGET: u32 = 0;
pub const FINISH_STOP: u32 = 1;
/// `Batch::generate_topp`: a top-p row's step found no candidate above the cutoff (`LMRS_FINISH_NO_CANDIDATE`).
pub const FINISH_NO_CANDIDATE: u32 = 2;

/// What `Batch::generate` returns: per row its tokens (cut to `n_out`), their log-probabilities when asked for, and its finish code; the passes the
/// loop ran, the sum over them of the rows in the pass, and the call's host wall time.
#[derive(Clone, Debug, Default)]
pub struct Generated {
    pub tokens: Vec<Vec<u32>>,
    pub logprobs: Vec<Vec<f32>>,
    pub finish: Vec<u32>,
    pub passes: u64,
    pub row_passes: u64,
    /// Host wall time of the call, in seconds.
    pub seconds: f64,
}

/// The record's word for a position whose token is unknown, or an embedding row (`LMRS_TOKEN_NONE`).
pub const TOKEN_NONE: u32 = 0xFFFF_FFFF;

/// A slot's penalties (`Batch::set_penalties`): tokens the slot has seen anywhere are divided / multiplied by `repetition`, tokens seen at positions
/// `>= out_from` lose `frequency * count + presence` (include/lmrs_hip.h: the rule).
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct Penalty {
    pub repetition: f32,
    pub presence: f32,
    pub frequency: f32,
    pub out_from: u32,
}

/// What a run of `Batch::forward_runs_embed` feeds: token ids, or rows of `dim` floats taken as `Transformer::fill_kv_cache` takes them.
pub enum RunRows<'r> {
    Tokens(&'r [u32]),
    Embeddings(&'r [f32]),
}

/// One run of `Batch::forward_runs_embed`: `rows` at `start_pos ..` of `slot`, outputs for its last `n_out` rows.
pub struct EmbedRun<'r> {
    pub slot: u32,
    pub start_pos: u32,
    pub rows: RunRows<'r>,
    pub n_out: u32,
}

/// One run of `Batch::forward_runs_sample`: `tokens` at `start_pos ..` of `slot`; `sampler`: the run's last row is sampled with it, `None`: K/V rows only.
pub struct SampledRun<'r, 's> {
    pub slot: u32,
    pub start_pos: u32,
    pub tokens: &'r [u32],
    pub sampler: Option<&'s mut Sampler>,
}

/// `fork`'s source: the transformer's own cache.
pub const BATCH_CTX: u32 = 0xFFFF_FFFF;

pub struct Batch<'t, 'a> {
    b: *mut LmrsBatch,
    vocab_size: usize,
    _t: &'t mut Transformer<'a>,
}

impl<'t, 'a> Batch<'t, 'a> {
    pub fn new(t: &'t mut Transformer<'a>, n_slots: u32) -> Batch<'t, 'a> {
        let mut b: *mut LmrsBatch = ptr::null_mut();
        check(unsafe { ffi::lmrs_batch_create(t.ctx(), n_slots, &mut b) });
        let vocab_size = t.args.vocab_size as usize;
        Batch { b, vocab_size, _t: t }
    }

    /// Up to 64 slots, and up to 64 rows a call of `forward` / `generate_greedy` (`forward_sample` keeps 16).
    pub fn new_wide(t: &'t mut Transformer<'a>, n_slots: u32) -> Batch<'t, 'a> {
        let mut b: *mut LmrsBatch = ptr::null_mut();
        check(unsafe { lmrs_batch_create_wide(t.ctx(), n_slots, &mut b) });
        let vocab_size = t.args.vocab_size as usize;
        Batch { b, vocab_size, _t: t }
    }

    /// A wide batch whose slots draw pages of `page_len` positions (64, 128, 256, 512 or 1024) from one pool of `n_pages` pages: `fork` shares whole
    /// pages, a write un-shares the page it touches, `release` gives pages back.  Without `release` every result is a wide batch's, bit for bit.
    pub fn new_paged(t: &'t mut Transformer<'a>, n_slots: u32, page_len: u32, n_pages: u32) -> Batch<'t, 'a> {
        let mut b: *mut LmrsBatch = ptr::null_mut();
        check(unsafe { lmrs_batch_create_paged(t.ctx(), n_slots, page_len, n_pages, &mut b) });
        let vocab_size = t.args.vocab_size as usize;
        Batch { b, vocab_size, _t: t }
    }

    /// A paged batch's pool: (page_len, n_pages, n_free).
    pub fn pages(&self) -> (u32, u32, u32) {
        let (mut l, mut n, mut f) = (0u32, 0u32, 0u32);
        check(unsafe { lmrs_batch_pages(self.b, &mut l, &mut n, &mut f) });
        (l, n, f)
    }

    /// The pages `slot` holds and how many of them have more than one holder: (held, shared).
    pub fn slot_pages(&self, slot: u32) -> (u32, u32) {
        let (mut h, mut s) = (0u32, 0u32);
        check(unsafe { lmrs_batch_slot_pages(self.b, slot, &mut h, &mut s) });
        (h, s)
    }

    /// Keep positions `[0, n_pos)` of `slot` (0 empties it); the pages behind them return to the pool once nobody holds them.
    pub fn release(&mut self, slot: u32, n_pos: u32) {
        check(unsafe { lmrs_batch_release(self.b, slot, n_pos) });
    }

    /// How `prefill` / `prefill_embeddings` would run `n` rows at `start_pos`: (passes of at most 512 rows, how many of them take block attention -
    /// 64-query blocks; the others take one workgroup per (head, row)).  Host arithmetic only, on any batch.
    pub fn prefill_form(&self, n: usize, start_pos: u32) -> (u32, u32) {
        let (mut c, mut k) = (0u32, 0u32);
        check(unsafe { lmrs_batch_prefill_form(self.b, n, start_pos, &mut c, &mut k) });
        (c, k)
    }

    /// Test / A-B aid: every prompt chunk of this paged batch takes the table pass from now on (`false`: the library's rule).  Panics on a batch that
    /// is not paged.
    pub fn debug_prefill_table(&mut self, force: bool) {
        check(unsafe { lmrs_batch_debug_prefill_table(self.b, force as c_int) });
    }

    /// The most rows a call takes: 16, or 64 for a wide batch.
    pub fn width(&self) -> u32 {
        let mut w = 0u32;
        check(unsafe { lmrs_batch_width(self.b, &mut w) });
        w
    }

    /// Penalties for `slot[i]`, state of the slots until replaced or cleared: every output of their rows in any call here comes from the row's logits
    /// changed over the tokens the slot has seen.  The first call switches the batch's token record on.
    pub fn set_penalties(&mut self, slot: &[u32], penalties: &[Penalty]) {
        assert!(slot.len() == penalties.len(), "one Penalty per slot");
        let rep: Vec<f32> = penalties.iter().map(|p| p.repetition).collect();
        let pres: Vec<f32> = penalties.iter().map(|p| p.presence).collect();
        let freq: Vec<f32> = penalties.iter().map(|p| p.frequency).collect();
        let from: Vec<u32> = penalties.iter().map(|p| p.out_from).collect();
        check(unsafe { lmrs_batch_set_penalties(self.b, slot.len() as u32, slot.as_ptr(), rep.as_ptr(), pres.as_ptr(), freq.as_ptr(), from.as_ptr()) });
    }

    /// The named slots lose their penalties; an empty list: every slot.
    pub fn clear_penalties(&mut self, slot: &[u32]) {
        check(unsafe { lmrs_batch_clear_penalties(self.b, slot.len() as u32, if slot.is_empty() { ptr::null() } else { slot.as_ptr() }) });
    }

    /// `slot`'s penalties as set, and whether they change a logit.
    pub fn penalty_info(&self, slot: u32) -> (Penalty, bool) {
        let (mut p, mut active) = (Penalty { repetition: 1.0, presence: 0.0, frequency: 0.0, out_from: 0 }, 0 as c_int);
        check(unsafe { lmrs_batch_penalty_info(self.b, slot, &mut p.repetition, &mut p.presence, &mut p.frequency, &mut p.out_from, &mut active) });
        (p, active != 0)
    }

    /// Filters for `slot[i]`, state of the slots until replaced or cleared; `(0, INFINITY)` is the same as clearing.
    pub fn set_filters(&mut self, slot: &[u32], filters: &[Filter]) {
        assert!(slot.len() == filters.len(), "one Filter per slot");
        let k: Vec<u32> = filters.iter().map(|f| f.top_k).collect();
        let gap: Vec<f32> = filters.iter().map(|f| f.min_gap).collect();
        check(unsafe { lmrs_batch_set_filters(self.b, slot.len() as u32, slot.as_ptr(), k.as_ptr(), gap.as_ptr()) });
    }

    /// The named slots lose their filters; an empty list: every slot.
    pub fn clear_filters(&mut self, slot: &[u32]) {
        check(unsafe { lmrs_batch_clear_filters(self.b, slot.len() as u32, if slot.is_empty() { ptr::null() } else { slot.as_ptr() }) });
    }

    /// `slot`'s filters as set, and whether they can clear a logit.
    pub fn filter_info(&self, slot: u32) -> (Filter, bool) {
        let (mut f, mut active) = (Filter { top_k: 0, min_gap: f32::INFINITY }, 0 as c_int);
        check(unsafe { lmrs_batch_filter_info(self.b, slot, &mut f.top_k, &mut f.min_gap, &mut active) });
        (f, active != 0)
    }

    /// The token record of `slot` from `start_pos` on = `tokens` (`TOKEN_NONE`: unknown); no tokens: only switches the record on.
    pub fn set_history(&mut self, slot: u32, tokens: &[u32], start_pos: u32) {
        check(unsafe { lmrs_batch_set_history(self.b, slot, start_pos, if tokens.is_empty() { ptr::null() } else { tokens.as_ptr() }, tokens.len()) });
    }

    /// The token record of `slot` at positions `start_pos .. start_pos + n`; panics on a batch that keeps no record.
    pub fn history(&mut self, slot: u32, n: usize, start_pos: u32) -> Vec<u32> {
        let mut out = vec![0u32; n];
        check(unsafe { lmrs_batch_history(self.b, slot, start_pos, n, if n == 0 { ptr::null_mut() } else { out.as_mut_ptr() }) });
        out
    }

    /// `Transformer::prefill_tokens` into `slot`'s cache.
    pub fn prefill(&mut self, slot: u32, tokens: &[u32], start_pos: u32) {
        check(unsafe { ffi::lmrs_batch_prefill(self.b, slot, tokens.as_ptr(), tokens.len(), start_pos) });
    }

    /// ONE `Transformer::fill_kv_cache` call into `slot`'s cache: `embeddings.len() / dim` rows, taken as given, from `start_pos` on.  With
    /// `residual` the rows come back as the reference leaves them in its mutated argument; without it nothing is downloaded.
    pub fn prefill_embeddings(&mut self, slot: u32, embeddings: &[f32], dim: usize, start_pos: u32, residual: Option<&mut [f32]>) {
        assert!(dim > 0 && embeddings.len() % dim == 0, "whole rows of dim floats");
        let rp = match residual {
            Some(r) => {
                assert!(r.len() == embeddings.len(), "residual holds as many floats as embeddings");
                r.as_mut_ptr()
            }
            None => ptr::null_mut(),
        };
        check(unsafe { lmrs_batch_prefill_embeddings(self.b, slot, embeddings.as_ptr(), (embeddings.len() / dim) as u32, start_pos, rp) });
    }

    /// One weight pass over runs of tokens and runs of embedding rows (`dim` floats a row), one run per slot: the argmax of every output row, in run
    /// order.  Row j of an embedding run is `fill_kv_cache(&row, 1, start_pos + j)` on a transformer that holds only that sequence.
    pub fn forward_runs_embed(&mut self, runs: &[EmbedRun], dim: usize) -> Vec<u32> {
        let (mut slot, mut start, mut len, mut n_out, mut kind) = (Vec::new(), Vec::new(), Vec::new(), Vec::new(), Vec::new());
        let (mut tokens, mut embeddings): (Vec<u32>, Vec<f32>) = (Vec::new(), Vec::new());
        for r in runs.iter() {
            slot.push(r.slot);
            start.push(r.start_pos);
            n_out.push(r.n_out);
            match r.rows {
                RunRows::Tokens(t) => {
                    len.push(t.len() as u32);
                    kind.push(0u32);
                    tokens.extend_from_slice(t);
                }
                RunRows::Embeddings(e) => {
                    assert!(dim > 0 && e.len() % dim == 0, "whole rows of dim floats");
                    len.push((e.len() / dim) as u32);
                    kind.push(1u32);
                    embeddings.extend_from_slice(e);
                }
            }
        }
        let outs: usize = n_out.iter().map(|&n| n as usize).sum();
        let mut argmax = vec![0u32; outs];
        let tp = if tokens.is_empty() { ptr::null() } else { tokens.as_ptr() };
        let ep = if embeddings.is_empty() { ptr::null() } else { embeddings.as_ptr() };
        let ap = if outs > 0 { argmax.as_mut_ptr() } else { ptr::null_mut() };
        check(unsafe {
            lmrs_batch_forward_runs_embed(self.b, runs.len() as u32, slot.as_ptr(), start.as_ptr(), len.as_ptr(), n_out.as_ptr(), kind.as_ptr(), tp, ep, ap,
                                          ptr::null_mut(), 0, ptr::null_mut(), ptr::null_mut())
        });
        argmax
    }

    /// K/V rows `[0, n_pos)` of `src` (`BATCH_CTX`: the transformer's own cache) into `dst`.
    pub fn fork(&mut self, src: u32, dst: u32, n_pos: u32) {
        check(unsafe { ffi::lmrs_batch_fork(self.b, src, dst, n_pos) });
    }

    /// One weight pass: row i = forward(tokens[i], pos[i]) on slot[i].  Returns the argmax of every row and, if asked, the n x vocab logits.
    pub fn forward(&mut self, slot: &[u32], tokens: &[u32], pos: &[u32], want_logits: bool) -> (Vec<u32>, Vec<f32>) {
        assert!(slot.len() == tokens.len() && slot.len() == pos.len(), "one slot, token and position per row");
        let mut argmax = vec![0u32; slot.len()];
        let mut logits = vec![0f32; if want_logits { slot.len() * self.vocab_size } else { 0 }];
        let lp = if want_logits { logits.as_mut_ptr() } else { ptr::null_mut() };
        check(unsafe { ffi::lmrs_batch_forward(self.b, slot.len() as u32, slot.as_ptr(), tokens.as_ptr(), pos.as_ptr(), argmax.as_mut_ptr(), lp) });
        (argmax, logits)
    }

    /// `forward` with a sampler per row, sampled on the device: next[i] = `Transformer::forward_sample(tokens[i], pos[i], samplers[i])` on slot[i].
    /// Rows may mix samplers; a top-p sampler serves one row of a call (the `&mut` borrows already say so).
    pub fn forward_sample(&mut self, slot: &[u32], tokens: &[u32], pos: &[u32], samplers: &mut [&mut Sampler]) -> Vec<u32> {
        assert!(slot.len() == tokens.len() && slot.len() == pos.len() && slot.len() == samplers.len(), "one slot, token, position and sampler per row");
        let handles: Vec<*mut LmrsSampler> = samplers.iter().map(|s| s.handle).collect();
        let mut next = vec![0u32; slot.len()];
        check(unsafe {
            lmrs_batch_forward_sample(self.b, slot.len() as u32, slot.as_ptr(), tokens.as_ptr(), pos.as_ptr(), handles.as_ptr(), next.as_mut_ptr())
        });
        next
    }

    /// One weight pass over runs of consecutive tokens, one run per slot (a prompt to admit, one decode row; at most `width()` runs and 512 tokens),
    /// the last row of every run that has a sampler sampled on the device with it: next[i] = `Transformer::forward_sample` after the run's tokens on
    /// a transformer that holds only that sequence, 0 for a run without a sampler (a prompt chunk that is not the last).
    pub fn forward_runs_sample(&mut self, runs: &mut [SampledRun]) -> Vec<u32> {
        let (mut slot, mut start, mut len, mut tokens) = (Vec::new(), Vec::new(), Vec::new(), Vec::new());
        let mut handles: Vec<*mut LmrsSampler> = Vec::new();
        for r in runs.iter() {
            slot.push(r.slot);
            start.push(r.start_pos);
            len.push(r.tokens.len() as u32);
            tokens.extend_from_slice(r.tokens);
            handles.push(r.sampler.as_ref().map_or(ptr::null_mut(), |s| s.handle));
        }
        let mut next = vec![0u32; runs.len()];
        check(unsafe {
            lmrs_batch_forward_runs_sample(self.b, runs.len() as u32, slot.as_ptr(), start.as_ptr(), len.as_ptr(), tokens.as_ptr(), handles.as_ptr(),
                                           next.as_mut_ptr())
        });
        next
    }

    /// `n_new` greedy steps of every row on the device: out[i * n_new + j].
    pub fn generate_greedy(&mut self, slot: &[u32], tokens: &[u32], pos: &[u32], n_new: u32) -> Vec<u32> {
        assert!(slot.len() == tokens.len() && slot.len() == pos.len(), "one slot, token and position per row");
        let mut out = vec![0u32; slot.len() * n_new as usize];
        check(unsafe {
            ffi::lmrs_batch_generate_greedy(self.b, slot.len() as u32, slot.as_ptr(), tokens.as_ptr(), pos.as_ptr(), n_new, out.as_mut_ptr(), ptr::null_mut())
        });
        out
    }

    /// The device loop whose rows end one by one (`lmrs_batch_generate`): row i feeds `tokens[i]` at `pos[i]` of `slot[i]` and goes on with what it
    /// chose - `Sampler::sample` with `samplers[i]`, the argmax for `None` or an empty list - until it chooses a token of `stop[i]` (`FINISH_STOP`; the
    /// token is reported, never fed) or has produced `max_new[i]` tokens (`FINISH_BUDGET`).  `stop`: empty, or one set of at most `STOP_MAX` tokens per
    /// row.  Argmax and sample_mult samplers only (they are stateless and may be shared); a top-p sampler panics with the library's message.
    /// `check_every`: passes between two looks at the rows' state; no result depends on it.
    #[allow(clippy::too_many_arguments)]
    pub fn generate(&mut self, slot: &[u32], tokens: &[u32], pos: &[u32], max_new: &[u32], stop: &[&[u32]], samplers: &[Option<&Sampler>],
                    check_every: u32, logprobs: bool) -> Generated {
        self.generate_by(false, slot, tokens, pos, max_new, stop, samplers, check_every, logprobs)
    }

    /// `generate` with top-p samplers admitted, each in one row only (`lmrs_batch_generate_topp`): their candidate vectors live on the device for the
    /// length of the call and are back in the samplers when it returns, so whatever is done with a sampler next continues exactly.  A row whose step
    /// finds no candidate above the cutoff ends with `FINISH_NO_CANDIDATE` and reports no token for that step.
    #[allow(clippy::too_many_arguments)]
    pub fn generate_topp(&mut self, slot: &[u32], tokens: &[u32], pos: &[u32], max_new: &[u32], stop: &[&[u32]], samplers: &[Option<&Sampler>],
                         check_every: u32, logprobs: bool) -> Generated {
        self.generate_by(true, slot, tokens, pos, max_new, stop, samplers, check_every, logprobs)
    }

    #[allow(clippy::too_many_arguments)]
    fn generate_by(&mut self, topp: bool, slot: &[u32], tokens: &[u32], pos: &[u32], max_new: &[u32], stop: &[&[u32]], samplers: &[Option<&Sampler>],
                   check_every: u32, logprobs: bool) -> Generated {
        let n = slot.len();
        assert!(tokens.len() == n && pos.len() == n && max_new.len() == n, "one slot, token, position and budget per row");
        assert!(stop.is_empty() || stop.len() == n, "stop is empty or holds one set per row");
        assert!(samplers.is_empty() || samplers.len() == n, "samplers is empty or holds one entry per row");
        let n_stop: Vec<u32> = stop.iter().map(|s| s.len() as u32).collect();
        let packed: Vec<u32> = stop.iter().flat_map(|s| s.iter().copied()).collect();
        let handles: Vec<*mut LmrsSampler> = samplers.iter().map(|s| s.map_or(ptr::null_mut(), |s| s.handle)).collect();
        let m = max_new.iter().copied().max().unwrap_or(0).max(1) as usize;
        let (mut out, mut lp) = (vec![0u32; n * m], vec![0f32; if logprobs { n * m } else { 0 }]);
        let (mut n_out, mut finish, mut stats, mut seconds) = (vec![0u32; n], vec![0u32; n], [0u64; 2], 0f64);
        let call = if topp { lmrs_batch_generate_topp } else { lmrs_batch_generate };
        check(unsafe {
            call(self.b, n as u32, slot.as_ptr(), tokens.as_ptr(), pos.as_ptr(), max_new.as_ptr(),
                 if stop.is_empty() { ptr::null() } else { n_stop.as_ptr() }, if packed.is_empty() { ptr::null() } else { packed.as_ptr() },
                 if samplers.is_empty() { ptr::null() } else { handles.as_ptr() }, check_every, out.as_mut_ptr(),
                 if logprobs { lp.as_mut_ptr() } else { ptr::null_mut() }, n_out.as_mut_ptr(), finish.as_mut_ptr(), stats.as_mut_ptr(),
                 &mut seconds)
        });
        let cut = |i: usize| i * m..i * m + n_out[i] as usize;
        Generated {
            tokens: (0..n).map(|i| out[cut(i)].to_vec()).collect(),
            logprobs: if logprobs { (0..n).map(|i| lp[cut(i)].to_vec()).collect() } else { Vec::new() },
            finish,
            passes: stats[0],
            row_passes: stats[1],
            seconds,
        }
    }
}

impl<'t, 'a> Drop for Batch<'t, 'a> {
    fn drop(&mut self) {
        unsafe { ffi::lmrs_batch_destroy(self.b) }
    }
}
