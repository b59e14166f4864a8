// lmrs_switches.h - the library's environment switches, read by read_switches alone: when a context, a CLIP tower or a tokenizer is
// created, and by lmrs_shard_plan (no context).  Flags are on when the variable is set at all (=0 included).  tests/test_docs.py checks
// that every switch has a row in INTEGRATION.md's table and that no other code under lm.rs_amd/csrc reads the environment.  Host-only C++.
#pragma once
#include <stdlib.h>
#include <string.h>

namespace lmrs {

constexpr int kAttLdsKeys = 2048;        // longest context whose block-softmax scores stay in LDS (launch_attention_block)

struct Switches {
    bool no_batched_prefill = false;     // LMRS_NO_BATCHED_PREFILL: fill_kv_cache and prompts go token by token through the decode kernels
    int tokens_batch_min = 0;            // LMRS_TOKENS_BATCH_MIN: shortest run of tokens lmrs_prefill_tokens / a prompt batches (0: the measured default; tools/prompt_rate.py)
    bool no_graph = false;               // LMRS_NO_GRAPH: a step's launches enqueued one by one (profiling aid, see launch_step)
    bool debug_timeline = false;         // LMRS_DEBUG_TIMELINE: in-kernel wall-clock stamps
    bool shard_f32_payload = false;      // LMRS_SHARD_F32_PAYLOAD: row shards exchange f32 slices
    bool group_p2p = false;              // LMRS_GROUP_P2P: a lock-step group exchanges through the push kernel
    bool att_long_batch_forms = false;   // LMRS_ATT_LONG_BATCH_FORMS: Gemma-2's block attention in its long-batch forms at any length (tests)
    bool vis_no_stray = false;           // LMRS_VIS_NO_STRAY: the CLIP tower's 577th query as a tenth block of 64 lanes (A/B aid, tests)
    int shard_plan = 0;                  // LMRS_SHARD_PLAN: 0 unset (chosen by bytes), 1 "cls", 2 any other value ("tp")
    bool shard_split_out = false;        // LMRS_SHARD_SPLIT_OUT != 0: wo / w2 row-split too
    int qkv_att = -1;                    // LMRS_QKV_ATT: -1 unset; 0 no merged qkv + attention launch; 1 its workgroup form only
    bool cls_tail = true;                // LMRS_CLS_TAIL=0: the final argmax as a launch of its own
    int att_split_pos = 384; bool att_split_pos_set = false;   // LMRS_ATT_SPLIT_POS: split attention from this position (0: never); set: used by stamped contexts too
    bool att_split_merged = true;        // LMRS_ATT_SPLIT_MERGED=0: the split form as six launches per layer (plain qkv, scores, values) - the A/B switch of the merged qkv + scores launch
    int att_split_score_wgs = 0;         // LMRS_ATT_SPLIT_SCORE_WGS: at most this many score workgroups in the merged qkv + scores launch (0: as many as are resident; tests lower it)
    int att_lds_keys = kAttLdsKeys;      // LMRS_ATT_LDS_KEYS (tests lower it)
    int steps_per_graph = 4;             // LMRS_STEPS_PER_GRAPH, clamped to 1 .. 64
    size_t topp_sort_min = 4096;         // LMRS_TOPP_DEVICE_SORT_MIN: device sort of top-p candidates from this count (host: 4096 in ~0.25 ms, device ~0.2 ms)
    long long p2p_timeout_ms = 3000;     // LMRS_P2P_TIMEOUT_MS
    int bsearch_flavour = 0;             // LMRS_BSEARCH_FLAVOUR
};

inline Switches read_switches() {
    Switches s;
    const char* e;
    s.no_batched_prefill = getenv("LMRS_NO_BATCHED_PREFILL") != nullptr;
    if ((e = getenv("LMRS_TOKENS_BATCH_MIN"))) { const int k = atoi(e); s.tokens_batch_min = k < 2 ? 2 : k; }
    s.no_graph = getenv("LMRS_NO_GRAPH") != nullptr;
    s.debug_timeline = getenv("LMRS_DEBUG_TIMELINE") != nullptr;
    s.shard_f32_payload = getenv("LMRS_SHARD_F32_PAYLOAD") != nullptr;
    s.group_p2p = getenv("LMRS_GROUP_P2P") != nullptr;
    s.att_long_batch_forms = getenv("LMRS_ATT_LONG_BATCH_FORMS") != nullptr;
    s.vis_no_stray = getenv("LMRS_VIS_NO_STRAY") != nullptr;
    if ((e = getenv("LMRS_SHARD_PLAN"))) s.shard_plan = strcmp(e, "cls") ? 2 : 1;
    if ((e = getenv("LMRS_SHARD_SPLIT_OUT"))) s.shard_split_out = atoi(e) != 0;
    if ((e = getenv("LMRS_QKV_ATT"))) s.qkv_att = atoi(e);
    if ((e = getenv("LMRS_CLS_TAIL"))) s.cls_tail = atoi(e) != 0;
    if ((e = getenv("LMRS_ATT_SPLIT_POS"))) { s.att_split_pos = atoi(e); s.att_split_pos_set = true; }
    if ((e = getenv("LMRS_ATT_SPLIT_MERGED"))) s.att_split_merged = atoi(e) != 0;
    if ((e = getenv("LMRS_ATT_SPLIT_SCORE_WGS"))) { const int k = atoi(e); s.att_split_score_wgs = k < 0 ? 0 : k; }
    if ((e = getenv("LMRS_ATT_LDS_KEYS"))) s.att_lds_keys = atoi(e);
    if ((e = getenv("LMRS_STEPS_PER_GRAPH"))) { const int k = atoi(e); s.steps_per_graph = k < 1 ? 1 : (k > 64 ? 64 : k); }
    if ((e = getenv("LMRS_TOPP_DEVICE_SORT_MIN"))) s.topp_sort_min = (size_t)atol(e);
    if ((e = getenv("LMRS_P2P_TIMEOUT_MS"))) s.p2p_timeout_ms = atoll(e);
    if ((e = getenv("LMRS_BSEARCH_FLAVOUR"))) s.bsearch_flavour = atoi(e);
    return s;
}

}  // namespace lmrs
