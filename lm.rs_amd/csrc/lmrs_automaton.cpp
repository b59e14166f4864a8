// lmrs_automaton.cpp — the token automaton's host side (lmrs_automaton.h): the check of a caller's tables and the walk over them.
// Plain C++ with no HIP in it; failures go through the library's one message slot (lmrs::text_fail, as lmrs_text.cpp's).
#include "lmrs_automaton.h"

#include <string>
#include <vector>

#include "../../include/lmrs_hip.h"

namespace lmrs {

int text_fail(const char* msg);
static int fail_s(const std::string& m) { return text_fail(m.c_str()); }

static_assert(LMRS_STATE_DEAD == kStateDead, "the header's DEAD is the tables'");

int automaton_check(const char* what_c, const AutomatonTables& t, uint32_t* n_allowed_out, bool ranges_only) {
    const std::string what = std::string(what_c) + ": ";
    if (!t.class_of || !t.next) return fail_s(what + "NULL argument (class_of / next)");
    if (t.vocab_size < 1) return fail_s(what + "vocab_size is 0");
    if (t.n_states < 1 || t.n_states >= kStateFinalBit) return fail_s(what + "n_states = " + std::to_string(t.n_states) + " is outside 1 .. 2^31 - 1");
    if (t.n_classes < 1 || t.n_classes > kClassesMax) return fail_s(what + "n_classes = " + std::to_string(t.n_classes) + " is outside 1 .. " + std::to_string(kClassesMax));
    std::vector<uint32_t> count;
    try { count.assign(t.n_classes, 0); } catch (...) { return fail_s(what + "out of memory"); }        // nothing may unwind through the C ABI
    for (uint32_t tok = 0; tok < t.vocab_size; ++tok) {
        const uint32_t c = t.class_of[tok];
        if (c >= t.n_classes) return fail_s(what + "token " + std::to_string(tok) + ": class " + std::to_string(c) + " is not below n_classes = " + std::to_string(t.n_classes));
        ++count[c];
    }
    for (uint32_t q = 0; q < t.n_states; ++q) {
        const uint32_t* row = t.next + (size_t)q * t.n_classes;
        uint32_t allowed = 0, live = 0, first_live = 0;
        for (uint32_t c = 0; c < t.n_classes; ++c) {
            if (row[c] == kStateDead) continue;
            if (row[c] >= t.n_states)
                return fail_s(what + "state " + std::to_string(q) + ", class " + std::to_string(c) + ": next = " + std::to_string(row[c]) + " is neither a state below n_states = " +
                              std::to_string(t.n_states) + " nor LMRS_STATE_DEAD");
            if (!live++) first_live = c;
            allowed += count[c];
        }
        if (!ranges_only && !allowed && !(t.final && t.final[q])) {
            if (!live) return fail_s(what + "state " + std::to_string(q) + " is not final and every class of it is dead: it allows no token");
            return fail_s(what + "state " + std::to_string(q) + " is not final and its live classes hold no token below vocab_size = " + std::to_string(t.vocab_size) + " (class " +
                          std::to_string(first_live) + " is empty): it allows no token");
        }
        if (n_allowed_out) n_allowed_out[q] = allowed;
    }
    return 0;
}

int automaton_walk(const char* what_c, const AutomatonTables& t, uint32_t state, const uint32_t* tokens, size_t n, uint32_t* out_state, size_t* n_walked) {
    const std::string what = std::string(what_c) + ": ";
    if (n_walked) *n_walked = 0;
    if (!t.class_of || !t.next || !out_state || !n_walked || (!tokens && n)) return fail_s(what + "NULL argument");
    if (t.n_states < 1 || t.n_classes < 1 || t.n_classes > kClassesMax) return fail_s(what + "n_states or n_classes out of range");
    if (state >= t.n_states) return fail_s(what + "state " + std::to_string(state) + " of " + std::to_string(t.n_states));
    *out_state = state;
    for (size_t i = 0; i < n; ++i) {
        if (tokens[i] >= t.vocab_size) return fail_s(what + "token " + std::to_string(i) + " = " + std::to_string(tokens[i]) + " is not below vocab_size = " + std::to_string(t.vocab_size));
        const uint32_t c = t.class_of[tokens[i]];
        const uint32_t nx = c < t.n_classes ? t.next[(size_t)state * t.n_classes + c] : kStateDead;
        if (nx == kStateDead || nx >= t.n_states)
            return fail_s(what + "token " + std::to_string(i) + " = " + std::to_string(tokens[i]) + " is not allowed in state " + std::to_string(state) + " (" + std::to_string(i) + " tokens walked)");
        state = nx;
        *out_state = state; *n_walked = i + 1;
    }
    return 0;
}

}  // namespace lmrs

extern "C" int lmrs_automaton_check(uint32_t vocab_size, uint32_t n_states, uint32_t n_classes, const uint16_t* class_of, const uint32_t* next, const uint8_t* final,
                                    uint32_t* n_allowed_out) {
    return lmrs::automaton_check("lmrs_automaton_check", lmrs::AutomatonTables{vocab_size, n_states, n_classes, class_of, next, final}, n_allowed_out, false);
}
extern "C" int lmrs_automaton_walk(uint32_t vocab_size, uint32_t n_states, uint32_t n_classes, const uint16_t* class_of, const uint32_t* next, const uint8_t* final,
                                   uint32_t state, const uint32_t* tokens, size_t n, uint32_t* out_state, size_t* n_walked) {
    return lmrs::automaton_walk("lmrs_automaton_walk", lmrs::AutomatonTables{vocab_size, n_states, n_classes, class_of, next, final}, state, tokens, n, out_state, n_walked);
}
