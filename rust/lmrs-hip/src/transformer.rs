//! `Transformer` (reference src/transformer.rs:127-131): `new` :134-314, `forward` :316-384, `get_embeddings` :659-669,
//! `fill_kv_cache` :672-684, `Drop` :688-712 - each a call into liblmrs_hip.so.  Weights, KV cache and activations live in HBM;
//! the mmap is only read while `new` uploads it.
use std::marker::PhantomData;
use std::ptr;

use memmap2::Mmap;

use crate::ffi::{self, check, LmrsCtx};

#[derive(Debug, Copy, Clone, PartialEq)]
#[repr(u8)]
pub enum ModelType {
    GEMMA = 0,
    LLAMA = 1,
    PHI = 2,
}

#[derive(Debug, Copy, Clone, PartialEq)]
#[repr(u8)]
pub enum QuantType {
    None = 0,
    Q8_0 = 1,
    Q4_0 = 2,
}

/// == `lmrs_args` of include/lmrs_hip.h (field for field; the file's packed header is decoded on the C side).
/// Public fields: the ones the reference exposes (`vocab_size`, `model_type`, `multimodal`, transformer.rs:66-73).
#[repr(C)]
#[derive(Debug, Copy, Clone)]
pub struct TransformerArgs {
    pub(crate) dim: u32,
    pub(crate) hidden_dim: u32,
    pub(crate) n_layers: u32,
    pub(crate) n_heads: u32,
    pub(crate) head_size: u32,
    pub(crate) n_kv_heads: u32,
    pub vocab_size: u32,
    pub(crate) seq_len: u32,
    pub(crate) rms_norm_eps: f32,
    pub(crate) rope_theta: f32,
    pub(crate) q_type: QuantType,
    pub model_type: ModelType,
    pub multimodal: bool,
    _pad: u8,
    pub(crate) group_size: u32,
}

pub struct ScoreTopk {
    pub logprobs: Vec<f32>,
    pub argmax: Vec<u32>,
    pub sum_logprob: f64,
    /// n x k, row t = the candidates of position t in rank order
    pub topk_idx: Vec<u32>,
    pub topk_logprob: Vec<f32>,
    pub target_rank: Vec<u32>,
}

pub struct Transformer<'a> {
    pub args: TransformerArgs,
    ctx: *mut LmrsCtx,
    _data: PhantomData<&'a Mmap>,
}

impl<'a> Transformer<'a> {
    /// transformer.rs:134 - returns the model and the number of bytes of `data` it covers (the offset of the vision
    /// section in a multimodal file).
    pub fn new(data: &'a Mmap) -> (Transformer<'a>, usize) {
        let mut ctx: *mut LmrsCtx = ptr::null_mut();
        let mut used: usize = 0;
        check(unsafe { ffi::lmrs_create(data.as_ptr(), data.len(), ffi::device(), &mut ctx, &mut used) });
        let args = unsafe { *ffi::lmrs_get_args(ctx) };
        (Transformer { args, ctx, _data: PhantomData }, used)
    }

    /// One process per GPU, rows of every weight matrix split over `world` GPUs (RCCL all-gathers over xGMI inside the
    /// step).  `unique_id`: the 128 bytes `comm_unique_id()` returned on rank 0, distributed by the launcher.
    pub fn new_sharded(data: &'a Mmap, rank: i32, world: i32, unique_id: &[u8; 128]) -> (Transformer<'a>, usize) {
        let mut ctx: *mut LmrsCtx = ptr::null_mut();
        let mut used: usize = 0;
        check(unsafe {
            ffi::lmrs_create_sharded(data.as_ptr(), data.len(), ffi::device(), rank, world, unique_id.as_ptr() as *const _, &mut ctx, &mut used)
        });
        let args = unsafe { *ffi::lmrs_get_args(ctx) };
        (Transformer { args, ctx, _data: PhantomData }, used)
    }

    /// transformer.rs:316 - the logits live in pinned host memory owned by the context and stay valid (and mutable: the
    /// reference's sampler scales them in place, sampler.rs:115-117) until the next call on `self`.
    pub fn forward(&mut self, token: u32, pos: u32) -> &mut [f32] {
        let mut p: *mut f32 = ptr::null_mut();
        check(unsafe { ffi::lmrs_forward(self.ctx, token, pos, &mut p) });
        unsafe { std::slice::from_raw_parts_mut(p, self.args.vocab_size as usize) }
    }

    /// `forward` followed by `Sampler::sample_argmax` (sampler.rs:29-41) on the device: no logits leave HBM.
    pub fn forward_argmax(&mut self, token: u32, pos: u32) -> u32 {
        let mut next: u32 = 0;
        check(unsafe { ffi::lmrs_forward_argmax(self.ctx, token, pos, &mut next) });
        next
    }

    /// transformer.rs:659
    pub fn get_embeddings(&self, tokens: &[u32]) -> Vec<f32> {
        let mut out = vec![0.0f32; tokens.len() * self.args.dim as usize];
        check(unsafe { ffi::lmrs_get_embeddings(self.ctx, tokens.as_ptr(), tokens.len(), out.as_mut_ptr()) });
        out
    }

    /// transformer.rs:672 - `embeddings` is updated in place exactly as the reference mutates its argument.
    pub fn fill_kv_cache(&mut self, embeddings: &mut [f32], curr_pos: u32) -> u32 {
        let n = embeddings.len() as u32 / self.args.dim;
        let mut new_pos: u32 = 0;
        check(unsafe { ffi::lmrs_fill_kv_cache(self.ctx, embeddings.as_mut_ptr(), n, curr_pos, &mut new_pos) });
        new_pos
    }

    pub(crate) fn ctx(&mut self) -> *mut LmrsCtx {
        self.ctx
    }

    /// The token loop of src/bin/chat.rs:188-222 at temperature 0, device-resident (one host sync per call): feeds `prompt`
    /// from position `start_pos`, then `n_new - 1` further steps feeding back the argmax; returns the `n_new` generated ids.
    pub fn generate_greedy(&mut self, prompt: &[u32], n_new: u32, start_pos: u32) -> Vec<u32> {
        let mut out = vec![0u32; n_new as usize];
        check(unsafe {
            ffi::lmrs_generate_greedy(self.ctx, prompt.as_ptr(), prompt.len(), n_new, start_pos, out.as_mut_ptr(), ptr::null_mut())
        });
        out
    }

    /// Extension (no reference counterpart): `forward` once per token of `tokens` from position `start_pos`, in one call.  Row t of
    /// the result (`vocab_size` logits each) is what `forward(tokens[t], start_pos + t)` returns after the calls for 0..t-1.
    pub fn forward_tokens(&mut self, tokens: &[u32], start_pos: u32) -> Vec<f32> {
        let mut out = vec![0.0f32; tokens.len() * self.args.vocab_size as usize];
        check(unsafe { ffi::lmrs_forward_tokens(self.ctx, tokens.as_ptr(), tokens.len(), start_pos, out.as_mut_ptr()) });
        out
    }

    /// Extension: the same pass with the logits kept on the device.  Returns (log softmax(logits_t)[tokens[t+1]] for t < n-1,
    /// `Sampler::sample_argmax` of every position, the sum of the log-probabilities in f64).
    pub fn score(&mut self, tokens: &[u32], start_pos: u32) -> (Vec<f32>, Vec<u32>, f64) {
        let mut logprobs = vec![0.0f32; tokens.len().saturating_sub(1)];
        let mut argmax = vec![0u32; tokens.len()];
        let mut sum: f64 = 0.0;
        check(unsafe {
            ffi::lmrs_score_tokens(self.ctx, tokens.as_ptr(), tokens.len(), start_pos, logprobs.as_mut_ptr(), argmax.as_mut_ptr(), &mut sum)
        });
        (logprobs, argmax, sum)
    }

    /// Extension: `score` with the `k` first next-token candidates of every position (1 <= k <= 256, k <= vocab_size), selected on the
    /// device.  Order: the larger logit first, equal logits by ascending index, NaNs last - a NaN at index 0 first, as `sample_argmax`
    /// has it, so rank 0 is `argmax[t]`.  `topk_logprob` shares the maximum and the sum of `logprobs`; `target_rank[t]` counts the
    /// candidates that precede `tokens[t+1]`, whatever `k` is.
    pub fn score_topk(&mut self, tokens: &[u32], k: u32, start_pos: u32) -> ScoreTopk {
        let n = tokens.len();
        let mut s = ScoreTopk {
            logprobs: vec![0.0f32; n.saturating_sub(1)],
            argmax: vec![0u32; n],
            sum_logprob: 0.0,
            topk_idx: vec![0u32; n * k as usize],
            topk_logprob: vec![0.0f32; n * k as usize],
            target_rank: vec![0u32; n.saturating_sub(1)],
        };
        check(unsafe {
            ffi::lmrs_score_tokens_topk(self.ctx, tokens.as_ptr(), n, start_pos, k, s.logprobs.as_mut_ptr(), s.argmax.as_mut_ptr(),
                                        &mut s.sum_logprob, s.topk_idx.as_mut_ptr(), s.topk_logprob.as_mut_ptr(), s.target_rank.as_mut_ptr())
        });
        s
    }

    /// Extension: `forward` followed by the selection of the `k` first candidates on the device, in `score_topk`'s order: (indices, their
    /// raw logits).  2k words cross to the host instead of `vocab_size` floats; the state afterwards is `forward`'s.
    pub fn forward_topk(&mut self, token: u32, pos: u32, k: u32) -> (Vec<u32>, Vec<f32>) {
        let mut idx = vec![0u32; k as usize];
        let mut val = vec![0.0f32; k as usize];
        check(unsafe { ffi::lmrs_forward_topk(self.ctx, token, pos, k, idx.as_mut_ptr(), val.as_mut_ptr()) });
        (idx, val)
    }

    /// Extension: `forward(tokens[t], start_pos + t)` for every t with the logits discarded - the K/V rows of a prompt from token ids,
    /// one batched pass on the device where `tokens_path` says so.  Returns `start_pos + tokens.len()`.
    pub fn prefill_tokens(&mut self, tokens: &[u32], start_pos: u32) -> u32 {
        let mut new_pos: u32 = 0;
        check(unsafe { ffi::lmrs_prefill_tokens(self.ctx, tokens.as_ptr(), tokens.len(), start_pos, &mut new_pos) });
        new_pos
    }

    /// Extension: `tokens[0]` is the last confirmed token at `start_pos`, `tokens[1..]` are drafts (2 <= n <= 16).  Returns (`forward_argmax`
    /// of every position, the number of leading drafts with `tokens[t + 1] == argmax[t]`), from one pass over the weights where `score`
    /// would run batched.  The next pass starts at `start_pos + n_accept + 1` with `argmax[n_accept]`.
    pub fn verify_tokens(&mut self, tokens: &[u32], start_pos: u32) -> (Vec<u32>, u32) {
        let mut argmax = vec![0u32; tokens.len()];
        let mut n_accept: u32 = 0;
        check(unsafe { ffi::lmrs_verify_tokens(self.ctx, tokens.as_ptr(), tokens.len(), start_pos, argmax.as_mut_ptr(), &mut n_accept) });
        (argmax, n_accept)
    }

    /// Extension: `generate_greedy`'s tokens, bit for bit, by prompt-lookup drafting (`draft_lookup`) and verify passes.  Returns (the `n_new`
    /// ids, [verify passes, drafted tokens, accepted tokens, plain decode steps]); passes + accepted + plain == n_new.
    pub fn generate_speculative(&mut self, prompt: &[u32], n_new: u32, start_pos: u32, max_draft: u32, ngram_max: u32) -> (Vec<u32>, [u32; 4]) {
        let mut out = vec![0u32; n_new as usize];
        let mut stats = [0u32; 4];
        check(unsafe {
            ffi::lmrs_generate_speculative(self.ctx, prompt.as_ptr(), prompt.len(), n_new, start_pos, max_draft, ngram_max, out.as_mut_ptr(),
                                           stats.as_mut_ptr(), ptr::null_mut())
        });
        (out, stats)
    }

    /// Whether `prefill_tokens` runs a run of `n` tokens as one batched pass on this context.
    pub fn tokens_path(&self, n: usize) -> bool {
        let mut batched: std::os::raw::c_int = 0;
        check(unsafe { ffi::lmrs_tokens_path(self.ctx, n, &mut batched) });
        batched != 0
    }
}

/// Prompt-lookup drafting, host only: the tokens that followed the latest earlier occurrence of the longest suffix of `hist` of at most
/// `ngram_max` tokens, at most `max_draft` of them (empty: no match).
pub fn draft_lookup(hist: &[u32], ngram_max: u32, max_draft: u32) -> Vec<u32> {
    let mut draft = vec![0u32; max_draft as usize];
    let mut n: u32 = 0;
    check(unsafe { ffi::lmrs_draft_lookup(hist.as_ptr(), hist.len(), ngram_max, max_draft, draft.as_mut_ptr(), &mut n) });
    draft.truncate(n as usize);
    draft
}

/// The communicator id rank 0 makes for `new_sharded`.
pub fn comm_unique_id() -> [u8; 128] {
    let mut id = [0u8; 128];
    check(unsafe { ffi::lmrs_comm_unique_id(id.as_mut_ptr() as *mut _) });
    id
}

impl<'a> Drop for Transformer<'a> {
    fn drop(&mut self) {
        unsafe { ffi::lmrs_destroy(self.ctx) }
    }
}

// one in-flight call per context (`&mut self`), contexts are independent
unsafe impl<'a> Send for Transformer<'a> {}
