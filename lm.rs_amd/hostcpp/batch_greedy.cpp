// batch_greedy.cpp — greedy continuations of up to 16 prompts at once (--wide: up to 64, a wide batch) (an extension; no reference counterpart): one prompt per line of --prompts,
// each tokenized with BOS (Tokenizer::encode, src/tokenizer.rs:66-151) and prefilled into a slot of its own (Batch::prefill: every token but the
// last), then --n greedy tokens of every prompt from one device loop (Batch::generate_greedy, lmrs_batch_generate_greedy): each step is ONE pass over
// the weights for all prompts.  Per prompt the ids are those of Transformer::generate_greedy on a context of its own.  Prints "[i] <continuation>"
// per prompt and a line with the aggregate rate.
//   usage: batch_greedy --model m.lmrs --tokenizer tokenizer.bin --prompts file.txt [--n N (default 64)] [--wide]
//   g++ -O2 -std=c++17 batch_greedy.cpp -I../../include -L.. -llmrs_hip -Wl,-rpath,'$ORIGIN/..' -o batch_greedy
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "text.hpp"

int main(int argc, char** argv) {
    std::string model_path, tok_path, prompts_path;
    long n_new = 64;
    bool wide = false;
    for (int i = 1; i < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--wide") { wide = true; --i; continue; }                  // (a switch: no value follows)
        if (i + 1 >= argc) { std::fprintf(stderr, "option %s needs a value\n", argv[i]); return 2; }
        if (k == "--model") model_path = argv[i + 1];
        else if (k == "--tokenizer") tok_path = argv[i + 1];
        else if (k == "--prompts") prompts_path = argv[i + 1];
        else if (k == "--n") n_new = std::atol(argv[i + 1]);
        else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (model_path.empty() || tok_path.empty() || prompts_path.empty() || n_new < 1) {
        std::fprintf(stderr, "usage: %s --model m.lmrs --tokenizer tokenizer.bin --prompts file.txt [--n N] [--wide]\n", argv[0]);
        return 2;
    }
    std::ifstream pf(prompts_path);
    if (!pf) { std::fprintf(stderr, "cannot read %s\n", prompts_path.c_str()); return 1; }
    std::vector<std::string> prompts;
    for (std::string line; prompts.size() < (wide ? 64u : 16u) && std::getline(pf, line);) if (!line.empty()) prompts.push_back(line);
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
        lmrs_host::Batch batch(model, n, wide);
        std::vector<std::uint32_t> slot(n), last(n), pos(n);
        for (std::uint32_t i = 0; i < n; ++i) {
            std::vector<std::uint32_t> ids = tok.encode(prompts[i], true, false, false, static_cast<lmrs_host::ModelType>(model.args.model_type));
            if (ids.size() + static_cast<std::size_t>(n_new) - 1 > model.args.seq_len) { std::fprintf(stderr, "prompt %u and %ld tokens exceed seq_len\n", i, n_new); return 1; }
            slot[i] = i; last[i] = ids.back(); pos[i] = static_cast<std::uint32_t>(ids.size() - 1);
            ids.pop_back();
            if (!ids.empty()) batch.prefill(i, ids, 0);                    // the last prompt token is the first row of the loop
        }
        double seconds = 0.0;
        const std::vector<std::uint32_t> out = batch.generate_greedy(slot, last, pos, static_cast<std::uint32_t>(n_new), &seconds);
        for (std::uint32_t i = 0; i < n; ++i) {
            std::string text;
            for (long j = 0; j < n_new; ++j) text += tok.decode(out[static_cast<std::size_t>(i) * n_new + j]);
            std::printf("[%u] %s\n", i, text.c_str());
        }
        std::printf("%u prompts x %ld tokens in %.3f ms: %.1f tok/s\n", n, n_new, seconds * 1e3, n * n_new / seconds);
    } catch (const lmrs_host::Panic& e) { std::fprintf(stderr, "panic: %s\n", e.what()); return 101; }
    return 0;
}
