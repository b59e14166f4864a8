// batch_tree.cpp — tree-speculative greedy decoding of up to 16 prompts at once (an extension; no reference counterpart): one prompt per line of --prompts,
// each tokenized with BOS and prefilled into a slot of its own.  Per step every slot drafts a small TREE of candidate continuations, one pass over the
// weights verifies all trees (Batch::forward_tree, lmrs_batch_forward_tree), the longest root-to-node path the model agrees with is accepted
// (Batch::tree_accept + Batch::accept_path) and becomes the slot's next positions.  The tree of a slot: node 0 is the token greedy decoding feeds next
// (known from the pass before, so at least one token is accepted per pass); under it the first branch is a prompt-lookup draft (Transformer::draft_lookup over
// prompt + output so far), and at each depth a sibling: the token the PREVIOUS pass ranked second (k = 2) for that same POSITION, where its first branch
// reached so far.  That guess is blind - the old row stood on a branch that was not accepted - so it is a demonstration of the tree call, not a drafter.
// The ids are exactly those of Batch::generate_greedy: acceptance only keeps tokens that are the argmax of the row before them.  Prints, per step and prompt, the
// accepted tokens and their number; then the continuations and the tokens accepted per pass.
//   usage: batch_tree --model m.lmrs --tokenizer tokenizer.bin --prompts file.txt [--n N (default 64)] [--draft D (default 4)]
//   g++ -O2 -std=c++17 batch_tree.cpp -I../../include -L.. -llmrs_hip -Wl,-rpath,'$ORIGIN/..' -o batch_tree
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "text.hpp"

int main(int argc, char** argv) {
    std::string model_path, tok_path, prompts_path;
    long n_new = 64, n_draft = 4;
    for (int i = 1; i + 1 < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--model") model_path = argv[i + 1];
        else if (k == "--tokenizer") tok_path = argv[i + 1];
        else if (k == "--prompts") prompts_path = argv[i + 1];
        else if (k == "--n") n_new = std::atol(argv[i + 1]);
        else if (k == "--draft") n_draft = std::atol(argv[i + 1]);
        else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (model_path.empty() || tok_path.empty() || prompts_path.empty() || n_new < 1 || n_draft < 0 || n_draft > 31) {
        std::fprintf(stderr, "usage: %s --model m.lmrs --tokenizer tokenizer.bin --prompts file.txt [--n N] [--draft D (0 .. 31)]\n", argv[0]);
        return 2;
    }
    std::ifstream pf(prompts_path);
    if (!pf) { std::fprintf(stderr, "cannot read %s\n", prompts_path.c_str()); return 1; }
    std::vector<std::string> prompts;
    for (std::string line; prompts.size() < 16u && std::getline(pf, line);) if (!line.empty()) prompts.push_back(line);
    if (prompts.empty()) { std::fprintf(stderr, "%s holds no prompt\n", prompts_path.c_str()); return 1; }
    const int fd = open(model_path.c_str(), O_RDONLY);
    if (fd < 0) { std::perror("open"); return 1; }
    struct stat st; fstat(fd, &st);
    void* m = mmap(nullptr, st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) { std::perror("mmap"); return 1; }
    try {
        using lmrs_host::Batch;
        auto [model, used] = lmrs_host::Transformer::create(static_cast<const std::uint8_t*>(m), st.st_size);
        (void)used;
        munmap(m, st.st_size); close(fd);                                  // (the weights are on the device now)
        lmrs_host::Tokenizer tok(tok_path);
        const std::uint32_t n = static_cast<std::uint32_t>(prompts.size());
        Batch batch(model, n);
        // per slot: prompt + output so far, the position the next tree hangs off, the output, and per POSITION the token the last pass ranked second for it
        std::vector<std::vector<std::uint32_t>> hist(n), out(n), alt(n, std::vector<std::uint32_t>(model.args.seq_len + 1, Batch::TREE_ROOT));
        std::vector<std::uint32_t> slot(n), last(n), pos(n);
        for (std::uint32_t i = 0; i < n; ++i) {
            hist[i] = tok.encode(prompts[i], true, false, false, static_cast<lmrs_host::ModelType>(model.args.model_type));
            if (hist[i].size() + static_cast<std::size_t>(n_new) + 2 * n_draft + 1 > model.args.seq_len) { std::fprintf(stderr, "prompt %u and %ld tokens exceed seq_len\n", i, n_new); return 1; }
            slot[i] = i; last[i] = hist[i].back(); pos[i] = static_cast<std::uint32_t>(hist[i].size() - 1);
            if (pos[i]) batch.prefill(i, std::vector<std::uint32_t>(hist[i].begin(), hist[i].end() - 1), 0);
        }
        const auto t0 = std::chrono::steady_clock::now();
        const std::vector<std::uint32_t> first = batch.forward(slot, last, pos);                // the row in front of the first tree
        for (std::uint32_t i = 0; i < n; ++i) { out[i].push_back(first[i]); hist[i].push_back(first[i]); ++pos[i]; }
        long passes = 1, accepted = n;
        for (long step = 0;; ++step) {
            std::vector<Batch::Tree> trees;
            std::vector<std::uint32_t> live, branch_len;
            for (std::uint32_t i = 0; i < n; ++i) {
                if (out[i].size() >= static_cast<std::size_t>(n_new)) continue;
                Batch::Tree t{i, pos[i], {Batch::TREE_ROOT}, {out[i].back()}};
                const std::vector<std::uint32_t> draft = lmrs_host::Transformer::draft_lookup(hist[i], 3, static_cast<std::uint32_t>(n_draft));
                for (std::uint32_t d = 0; d < draft.size(); ++d) { t.parents.push_back(d); t.tokens.push_back(draft[d]); }        // first branch: nodes 0 .. draft.size()
                const std::uint32_t chain = static_cast<std::uint32_t>(draft.size()) + 1;
                for (std::uint32_t d = 1; d < chain + 1; ++d) {                                   // a sibling at depth d, under the first branch's node d - 1
                    const std::uint32_t a = alt[i][pos[i] + d];
                    if (a != Batch::TREE_ROOT && (d >= chain || a != t.tokens[d])) { t.parents.push_back(d - 1); t.tokens.push_back(a); }
                }
                trees.push_back(t); live.push_back(i); branch_len.push_back(chain);
            }
            if (trees.empty()) break;
            const Batch::RunsOut o = batch.forward_tree(trees, 2);
            ++passes;
            std::vector<Batch::Path> paths;
            std::size_t r0 = 0;
            for (std::size_t u = 0; u < trees.size(); ++u) {
                const Batch::Tree& t = trees[u];
                const std::uint32_t i = live[u], nn = static_cast<std::uint32_t>(t.tokens.size());
                const std::vector<std::uint32_t> am(o.argmax.begin() + r0, o.argmax.begin() + r0 + nn);
                const auto [path, next] = Batch::tree_accept(t.parents, t.tokens, am, out[i].back());
                std::string text;
                for (std::uint32_t j : path) { out[i].push_back(am[j]); hist[i].push_back(am[j]); text += tok.decode(am[j]); }
                std::fill(alt[i].begin(), alt[i].end(), Batch::TREE_ROOT);                        // first-branch node d stands at pos + d and ranks position pos + d + 1
                for (std::uint32_t d = 0; d < branch_len[u]; ++d) alt[i][pos[i] + d + 1] = o.topk_idx[(r0 + d) * 2 + 1];
                std::printf("step %ld [%u] +%zu of %u nodes: %s\n", step, i, path.size(), nn, text.c_str());
                paths.push_back(Batch::Path{i, pos[i], path});
                pos[i] += static_cast<std::uint32_t>(path.size()); accepted += static_cast<long>(path.size());
                (void)next;
                r0 += nn;
            }
            batch.accept_path(paths);
        }
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        for (std::uint32_t i = 0; i < n; ++i) {
            std::string text;
            for (long j = 0; j < n_new; ++j) text += tok.decode(out[i][j]);
            std::printf("[%u] %s\n", i, text.c_str());
        }
        std::printf("%u prompts: %ld tokens in %ld passes (%.2f a pass and prompt) in %.3f ms: %.1f tok/s\n", n, accepted, passes,
                    static_cast<double>(accepted) / (passes * n), seconds * 1e3, accepted / seconds);
    } catch (const lmrs_host::Panic& e) { std::fprintf(stderr, "panic: %s\n", e.what()); return 101; }
    return 0;
}
