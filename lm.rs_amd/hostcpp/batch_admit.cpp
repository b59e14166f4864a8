// batch_admit.cpp — batch_greedy.cpp's continuations through the ragged pass (an extension; no reference counterpart): one prompt per line of --prompts (up to
// 16), each tokenized with BOS (Tokenizer::encode, src/tokenizer.rs:66-151).  ALL prompts are admitted in ONE call of Batch::forward_runs
// (lmrs_batch_forward_runs): every prompt is a run of its own slot whose last row gives the prompt's first new token - one pass over the weights, where
// batch_greedy prefills slot by slot.  The LAST prompt is the late one: only its first --chunk tokens ride in that call, the rest follows --chunk tokens a
// step as one more run BESIDE the decode rows of the running prompts, which never wait for it.  Every step is one pass; per prompt the ids are those of
// batch_greedy (and of Transformer::generate_greedy on a context of its own).  Prints "[i] <continuation>" per prompt and the number of passes.
//   usage: batch_admit --model m.lmrs --tokenizer tokenizer.bin --prompts file.txt [--n N (default 64)] [--chunk C (default 8)]
//   g++ -O2 -std=c++17 batch_admit.cpp -I../../include -L.. -llmrs_hip -Wl,-rpath,'$ORIGIN/..' -o batch_admit
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "text.hpp"

int main(int argc, char** argv) {
    std::string model_path, tok_path, prompts_path;
    long n_new = 64, chunk = 8;
    for (int i = 1; i + 1 < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--model") model_path = argv[i + 1];
        else if (k == "--tokenizer") tok_path = argv[i + 1];
        else if (k == "--prompts") prompts_path = argv[i + 1];
        else if (k == "--n") n_new = std::atol(argv[i + 1]);
        else if (k == "--chunk") chunk = std::atol(argv[i + 1]);
        else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (model_path.empty() || tok_path.empty() || prompts_path.empty() || n_new < 1 || chunk < 1) {
        std::fprintf(stderr, "usage: %s --model m.lmrs --tokenizer tokenizer.bin --prompts file.txt [--n N] [--chunk C]\n", argv[0]);
        return 2;
    }
    std::ifstream pf(prompts_path);
    if (!pf) { std::fprintf(stderr, "cannot read %s\n", prompts_path.c_str()); return 1; }
    std::vector<std::string> prompts;
    for (std::string line; prompts.size() < 16 && std::getline(pf, line);) if (!line.empty()) prompts.push_back(line);
    if (prompts.empty()) { std::fprintf(stderr, "%s holds no prompt\n", prompts_path.c_str()); return 1; }
    const int fd = open(model_path.c_str(), O_RDONLY);
    if (fd < 0) { std::perror("open"); return 1; }
    struct stat st; fstat(fd, &st);
    void* m = mmap(nullptr, st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) { std::perror("mmap"); return 1; }
    try {
        auto [model, used] = lmrs_host::Transformer::create(static_cast<const std::uint8_t*>(m), st.st_size);
        (void)used;
        munmap(m, st.st_size); close(fd);                                  // (the weights are on the device now)
        lmrs_host::Tokenizer tok(tok_path);
        const std::uint32_t n = static_cast<std::uint32_t>(prompts.size());
        lmrs_host::Batch batch(model, n);
        using Run = lmrs_host::Batch::Run;
        std::vector<std::vector<std::uint32_t>> ids(n), out(n);
        std::vector<std::size_t> fed(n, 0);                                // prompt tokens of sequence i already in its slot
        std::size_t total = 0;
        for (std::uint32_t i = 0; i < n; ++i) {
            ids[i] = tok.encode(prompts[i], true, false, false, static_cast<lmrs_host::ModelType>(model.args.model_type));
            if (ids[i].size() + static_cast<std::size_t>(n_new) - 1 > model.args.seq_len) { std::fprintf(stderr, "prompt %u and %ld tokens exceed seq_len\n", i, n_new); return 1; }
            total += ids[i].size();
        }
        if (total > 512) { std::fprintf(stderr, "the prompts hold %zu tokens, more than the 512 rows of one pass\n", total); return 1; }
        const std::uint32_t late = n > 1 ? n - 1 : n;                      // (one prompt: nobody to be late beside)
        long passes = 0;
        for (;; ++passes) {
            // a run per sequence that still has work: the rest of its prompt (the late one: a chunk of it), or its last new token
            std::vector<Run> runs;
            std::vector<std::uint32_t> who;                                 // the sequence behind every run that asks for an output
            for (std::uint32_t i = 0; i < n; ++i) {
                if (out[i].size() == static_cast<std::size_t>(n_new)) continue;
                Run r{i, 0, {}, 1};
                if (fed[i] < ids[i].size()) {
                    const std::size_t take = i == late ? std::min<std::size_t>(static_cast<std::size_t>(chunk), ids[i].size() - fed[i]) : ids[i].size() - fed[i];
                    r.start_pos = static_cast<std::uint32_t>(fed[i]);
                    r.tokens.assign(ids[i].begin() + static_cast<std::ptrdiff_t>(fed[i]), ids[i].begin() + static_cast<std::ptrdiff_t>(fed[i] + take));
                    fed[i] += take;
                    r.n_out = fed[i] == ids[i].size() ? 1 : 0;              // a chunk inside the prompt only leaves its K/V rows
                } else {
                    r.start_pos = static_cast<std::uint32_t>(ids[i].size() + out[i].size() - 1);
                    r.tokens.push_back(out[i].back());
                }
                if (r.n_out) who.push_back(i);
                runs.push_back(std::move(r));
            }
            if (runs.empty()) break;
            const lmrs_host::Batch::RunsOut o = batch.forward_runs(runs);
            for (std::size_t j = 0; j < who.size(); ++j) out[who[j]].push_back(o.argmax[j]);
        }
        for (std::uint32_t i = 0; i < n; ++i) {
            std::string text;
            for (std::uint32_t t : out[i]) text += tok.decode(t);
            std::printf("[%u] %s\n", i, text.c_str());
        }
        std::printf("%u prompts x %ld tokens in %ld passes over the weights\n", n, n_new, passes);
    } catch (const lmrs_host::Panic& e) { std::fprintf(stderr, "panic: %s\n", e.what()); return 101; }
    return 0;
}
