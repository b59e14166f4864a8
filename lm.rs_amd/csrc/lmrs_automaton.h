// lmrs_automaton.h — the token automaton of a batch slot on the host (lmrs_automaton_check / lmrs_automaton_walk, include/lmrs_hip.h): plain
// arithmetic over the caller's tables, no HIP in it.  lmrs_api.hip runs the same two functions under its own calls' names.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace lmrs {

constexpr uint32_t kStateDead = 0xFFFFFFFFu;                // = LMRS_STATE_DEAD
constexpr uint32_t kStateFinalBit = 0x80000000u;            // the device's `next` entries carry the successor's final flag here: n_states stays below 2^31
constexpr uint32_t kClassesMax = 65536;                     // class_of is uint16_t

// The tables of a DFA over tokens as the caller hands them over: class_of[vocab_size] < n_classes, next[n_states][n_classes] a state or kStateDead,
// final (may be null: no state is final) a flag per state
struct AutomatonTables {
    uint32_t vocab_size, n_states, n_classes;
    const uint16_t* class_of; const uint32_t* next; const uint8_t* final;
};
// Every rule of lmrs_automaton_check, each message opening with `what`; n_allowed_out (n_states, may be null) takes every state's allowed tokens.
// ranges_only: the tables' ranges alone - what a kernel that indexes by them needs - without the rule that a non-final state allows a token.
int automaton_check(const char* what, const AutomatonTables& t, uint32_t* n_allowed_out, bool ranges_only);
// tokens[0 .. n) from `state`: 0 and *out_state = the state behind them, *n_walked = n; at the first token the state does not allow -1, *out_state = the
// state in front of it and *n_walked = the tokens consumed.  The tables are taken as checked; arguments out of range fail with *n_walked = 0.
int automaton_walk(const char* what, const AutomatonTables& t, uint32_t state, const uint32_t* tokens, size_t n, uint32_t* out_state, size_t* n_walked);

}  // namespace lmrs
