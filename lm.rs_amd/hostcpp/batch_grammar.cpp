// batch_grammar.cpp — grammar-constrained rows inside the batch's device loop (an extension; no reference counterpart): token automata on batch slots
// (Batch::automaton / attach, lmrs_batch_automaton_create / lmrs_batch_attach_automaton).  Two automata are built on a wide batch of --rows rows that stand
// at --depth positions:
//   a TRIE over three labels of 1, 2 and 3 tokens ("choose one of these"): every row ends FINISH_FINAL with one of the labels, printed per row;
//   a CYCLIC automaton of --states states over two classes (even and odd token ids): state s allows the ids of parity s % 2 - half the vocabulary - and moves
//   to (s + 1) % states, so the mask changes with every token and no row ever ends before its budget.
// Under the cyclic automaton --n tokens a row are generated three ways, by turns, --rounds times each, and each form's median and spread are printed:
//   loop      ONE Batch::generate call: the boundary launch moves the slots' states on the device;
//   per-step  what a caller did without automata: per step a host walk, Batch::set_masks of every row's state (n_slots * W words up) and a one-token
//             Batch::generate call;
//   static    the same loop under constant masks of the same density (Batch::set_masks once): the difference to `loop` is the automaton's own cost.
// With --temperature T > 0 the rows sample with Sampler::new(vocab_size, T, 1.0, --seed + i) (sample_mult), else they take the argmax.  The three forms give the
// same tokens where they compute the same thing (loop and per-step); the program checks that and fails otherwise.
//   usage: batch_grammar --model m.lmrs [--rows R (16)] [--depth D (100)] [--n N (128)] [--states S (4)] [--rounds K (5)] [--check-every C (8)] [--temperature T (0)] [--seed S (0)]
//   g++ -O2 -std=c++17 batch_grammar.cpp -I../../include -L.. -llmrs_hip -Wl,-rpath,'$ORIGIN/..' -o batch_grammar
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "text.hpp"

using lmrs_host::Batch;
using u32 = std::uint32_t;

static double seconds_of(const std::chrono::steady_clock::time_point& t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

int main(int argc, char** argv) {
    std::string model_path;
    long rows = 16, depth = 100, n_new = 128, states = 4, rounds = 5, check_every = 8;
    float temperature = 0.0f;
    unsigned long long seed = 0;
    for (int i = 1; i < argc; i += 2) {
        const std::string k = argv[i];
        if (i + 1 >= argc) { std::fprintf(stderr, "option %s needs a value\n", argv[i]); return 2; }
        if (k == "--model") model_path = argv[i + 1];
        else if (k == "--rows") rows = std::atol(argv[i + 1]);
        else if (k == "--depth") depth = std::atol(argv[i + 1]);
        else if (k == "--n") n_new = std::atol(argv[i + 1]);
        else if (k == "--states") states = std::atol(argv[i + 1]);
        else if (k == "--rounds") rounds = std::atol(argv[i + 1]);
        else if (k == "--check-every") check_every = std::atol(argv[i + 1]);
        else if (k == "--temperature") temperature = std::strtof(argv[i + 1], nullptr);
        else if (k == "--seed") seed = std::strtoull(argv[i + 1], nullptr, 10);
        else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (model_path.empty() || rows < 1 || rows > 64 || depth < 1 || n_new < 1 || states < 1 || rounds < 1 || check_every < 1) {
        std::fprintf(stderr, "usage: %s --model m.lmrs [--rows R] [--depth D] [--n N] [--states S] [--rounds K] [--check-every C] [--temperature T] [--seed S]\n", argv[0]);
        return 2;
    }
    const int fd = open(model_path.c_str(), O_RDONLY);
    if (fd < 0) { std::perror("open"); return 1; }
    struct stat st; fstat(fd, &st);
    void* m = mmap(nullptr, st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) { std::perror("mmap"); return 1; }
    try {
        auto [model, used] = lmrs_host::Transformer::create(static_cast<const std::uint8_t*>(m), st.st_size);
        (void)used;
        munmap(m, st.st_size); close(fd);
        const u32 n = static_cast<u32>(rows), V = model.args.vocab_size, S = static_cast<u32>(states), N = static_cast<u32>(n_new);
        if (static_cast<std::size_t>(depth) + N > model.args.seq_len || depth > 512) { std::fprintf(stderr, "depth + n exceeds seq_len (or depth 512)\n"); return 1; }
        Batch batch(model, n, /*wide=*/true);
        const std::size_t W = batch.mask_words();
        std::vector<u32> slots(n), first(n), pos(n, static_cast<u32>(depth)), budget(n, N), one(n, 1u);
        for (u32 i = 0; i < n; ++i) {                    // the rows' prefixes: `depth` ids of a sequence of its own each, K/V rows only
            slots[i] = i; first[i] = (11u + 37u * i) % V;
            std::vector<u32> ids(static_cast<std::size_t>(depth));
            for (std::size_t j = 0; j < ids.size(); ++j) ids[j] = static_cast<u32>((1009u * i + 31u * j + 7u) % V);
            batch.forward_runs({Batch::Run{i, 0, ids, 0}});
        }
        std::vector<std::unique_ptr<lmrs_host::Sampler>> owners;
        std::vector<lmrs_sampler*> samplers;
        for (u32 i = 0; i < n && temperature > 0.0f; ++i) { owners.push_back(std::make_unique<lmrs_host::Sampler>(V, temperature, 1.0f, seed + i)); samplers.push_back(owners.back()->handle()); }

        // ---- the trie: labels {5}, {6, 7}, {6, 8, 9}; states 0 root, 1 behind 6, 2 behind 6 8, 3 .. 5 the leaves.  Classes: 0 every other token, 1 .. 5 the ids 5 .. 9
        {
            std::vector<std::uint16_t> class_of(V, 0);
            for (u32 t = 5; t <= 9 && t < V; ++t) class_of[t] = static_cast<std::uint16_t>(t - 4);
            std::vector<u32> next(6 * 6, Batch::STATE_DEAD);
            next[0 * 6 + 1] = 3; next[0 * 6 + 2] = 1; next[1 * 6 + 3] = 4; next[1 * 6 + 4] = 2; next[2 * 6 + 5] = 5;
            lmrs_automaton* trie = batch.automaton(6, 6, class_of, next, {0, 0, 0, 1, 1, 1});
            batch.attach(slots, std::vector<lmrs_automaton*>(n, trie), std::vector<u32>(n, 0u));
            const Batch::Generated g = batch.generate(slots, first, pos, std::vector<u32>(n, 8u), {}, samplers, 4);
            for (u32 i = 0; i < n; ++i) {
                std::string label;
                for (u32 t : g.tokens[i]) label += " " + std::to_string(t);
                std::printf("[%u] %s:%s\n", i, g.finish[i] == Batch::FINISH_FINAL ? "final" : "NOT FINAL", label.c_str());
                if (g.finish[i] != Batch::FINISH_FINAL) return 1;
            }
            batch.attach(slots, std::vector<lmrs_automaton*>(n, nullptr), std::vector<u32>(n, 0u));
            batch.drop_automaton(trie);
        }

        // ---- the cyclic automaton: two classes by the id's parity, state s allows parity s % 2 and moves on to (s + 1) % S
        std::vector<std::uint16_t> class_of(V);
        for (u32 t = 0; t < V; ++t) class_of[t] = static_cast<std::uint16_t>(t & 1u);
        std::vector<u32> next(static_cast<std::size_t>(S) * 2, Batch::STATE_DEAD);
        for (u32 s = 0; s < S; ++s) next[s * 2 + (s & 1u)] = (s + 1) % S;
        const auto t_create = std::chrono::steady_clock::now();
        lmrs_automaton* cyc = batch.automaton(S, 2, class_of, next);
        std::fprintf(stderr, "lmrs_batch_automaton_create, %u states: %.1f us\n", S, 1e6 * seconds_of(t_create));
        std::vector<u32> parity_bits[2];                 // the masks of the two parities, for the per-step and the static route
        for (u32 par = 0; par < 2; ++par) {
            parity_bits[par].assign(W, par ? 0xAAAAAAAAu : 0x55555555u);
            if (V % 32) parity_bits[par][W - 1] &= (1u << V % 32) - 1u;
        }
        std::vector<u32> start(n);
        for (u32 i = 0; i < n; ++i) start[i] = i % S;
        const std::vector<lmrs_automaton*> all(n, cyc), none(n, nullptr);
        std::vector<std::vector<u32>> loop_tokens;
        std::vector<double> t_loop, t_step, t_static;
        for (long r = 0; r < rounds; ++r) {
            // loop
            batch.clear_masks();
            batch.attach(slots, all, start);
            auto t0 = std::chrono::steady_clock::now();
            const Batch::Generated g = batch.generate(slots, first, pos, budget, {}, samplers, static_cast<u32>(check_every));
            t_loop.push_back(seconds_of(t0));
            loop_tokens = g.tokens;
            batch.attach(slots, none, start);
            // per-step: the host walks, uploads every row's mask and asks for one token
            std::vector<u32> last = first, at = pos, q = start, bits(n * W);
            std::vector<std::vector<u32>> step_tokens(n);
            t0 = std::chrono::steady_clock::now();
            for (u32 j = 0; j < N; ++j) {
                for (u32 i = 0; i < n; ++i) std::copy(parity_bits[q[i] & 1u].begin(), parity_bits[q[i] & 1u].end(), bits.begin() + i * W);
                batch.set_masks(slots, bits);
                const Batch::Generated s1 = batch.generate(slots, last, at, one, {}, samplers, 1);
                for (u32 i = 0; i < n; ++i) {
                    last[i] = s1.tokens[i][0]; ++at[i]; step_tokens[i].push_back(last[i]);
                    q[i] = next[q[i] * 2 + class_of[last[i]]];
                }
            }
            t_step.push_back(seconds_of(t0));
            if (step_tokens != loop_tokens) { std::fprintf(stderr, "round %ld: the loop and the per-step route disagree\n", r); return 1; }
            // static masks of the same density in the same loop
            for (u32 i = 0; i < n; ++i) std::copy(parity_bits[start[i] & 1u].begin(), parity_bits[start[i] & 1u].end(), bits.begin() + i * W);
            batch.set_masks(slots, bits);
            t0 = std::chrono::steady_clock::now();
            batch.generate(slots, first, pos, budget, {}, samplers, static_cast<u32>(check_every));
            t_static.push_back(seconds_of(t0));
        }
        auto report = [&](const char* name, std::vector<double> t) {
            std::sort(t.begin(), t.end());
            std::printf("%-8s %9.1f us a step (median of %zu; %.1f .. %.1f)\n", name, 1e6 * t[t.size() / 2] / N, t.size(), 1e6 * t.front() / N, 1e6 * t.back() / N);
            return t[t.size() / 2];
        };
        std::printf("%u rows at %ld positions, %u tokens a row, %u states, %s rows\n", n, depth, N, S, temperature > 0.0f ? "sample_mult" : "argmax");
        const double l = report("loop", t_loop), p = report("per-step", t_step), s = report("static", t_static);
        std::printf("per-step / loop = %.3f%s; loop - static = %.1f us a step\n", p / l, l <= p ? "" : " MISSED", 1e6 * (l - s) / N);
    } catch (const lmrs_host::Panic& e) { std::fprintf(stderr, "panic: %s\n", e.what()); return 101; }
    return 0;
}
