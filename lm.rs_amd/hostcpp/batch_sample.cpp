// batch_sample.cpp — sampled continuations of several prompts at once (an extension; no reference counterpart): one prompt per line of --prompts (up to
// 16), each tokenized with BOS (Tokenizer::encode, src/tokenizer.rs:66-151).  ALL prompts are admitted in ONE call of Batch::forward_runs
// (lmrs_batch_forward_runs: K/V rows only, but for each prompt's last token), then every step is ONE call of Batch::forward_sample
// (lmrs_batch_forward_sample): a pass over the weights and Sampler::sample per row on the device, row i with a sampler of its own - the reference's
// Sampler::new(vocab_size, --temperature, --top-p, --seed + i).  Per prompt the ids are those of Transformer::forward_sample with that sampler on a
// context of its own.  Prints "[i] id id id ..." per prompt.
// --wide: up to 64 prompts on a wide batch (lmrs_batch_create_wide), everything through Batch::forward_runs_sample (lmrs_batch_forward_runs_sample): the
// WHOLE prompts are admitted in one pass that also samples each prompt's first token, then every step is one call with runs of one token.  Same ids.
//   usage: batch_sample --model m.lmrs --tokenizer tokenizer.bin --prompts file.txt [--n N (default 64)] [--temperature T (0.7)] [--top-p P (0.9)] [--seed S (0)] [--wide]
//   g++ -O2 -std=c++17 batch_sample.cpp -I../../include -L.. -llmrs_hip -Wl,-rpath,'$ORIGIN/..' -o batch_sample
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>

#include "text.hpp"

int main(int argc, char** argv) {
    std::string model_path, tok_path, prompts_path;
    long n_new = 64;
    float temperature = 0.7f, top_p = 0.9f;                                // chat.rs:28-31
    unsigned long long seed = 0;
    bool wide = false;
    for (int i = 1; i < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--wide") { wide = true; --i; continue; }                 // (the one option without a value)
        if (i + 1 >= argc) { std::fprintf(stderr, "option %s needs a value\n", argv[i]); return 2; }
        if (k == "--model") model_path = argv[i + 1];
        else if (k == "--tokenizer") tok_path = argv[i + 1];
        else if (k == "--prompts") prompts_path = argv[i + 1];
        else if (k == "--n") n_new = std::atol(argv[i + 1]);
        else if (k == "--temperature") temperature = std::strtof(argv[i + 1], nullptr);
        else if (k == "--top-p") top_p = std::strtof(argv[i + 1], nullptr);
        else if (k == "--seed") seed = std::strtoull(argv[i + 1], nullptr, 10);
        else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (model_path.empty() || tok_path.empty() || prompts_path.empty() || n_new < 1) {
        std::fprintf(stderr, "usage: %s --model m.lmrs --tokenizer tokenizer.bin --prompts file.txt [--n N] [--temperature T] [--top-p P] [--seed S] [--wide]\n", argv[0]);
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
        if (wide) {
            // one sampler per prompt (seed + row); admission and first token in ONE pass, then one pass a step with runs of one token
            std::vector<std::unique_ptr<lmrs_host::Sampler>> samplers;
            std::vector<lmrs_host::Batch::SampledRun> runs;
            std::size_t total = 0;
            for (std::uint32_t i = 0; i < n; ++i) {
                std::vector<std::uint32_t> ids = tok.encode(prompts[i], true, false, false, static_cast<lmrs_host::ModelType>(model.args.model_type));
                if (ids.size() + static_cast<std::size_t>(n_new) - 1 > model.args.seq_len) { std::fprintf(stderr, "prompt %u and %ld tokens exceed seq_len\n", i, n_new); return 1; }
                total += ids.size();
                samplers.push_back(std::make_unique<lmrs_host::Sampler>(model.args.vocab_size, temperature, top_p, seed + i));
                runs.push_back(lmrs_host::Batch::SampledRun{i, 0, std::move(ids), samplers.back()->handle()});
            }
            if (total > 512) { std::fprintf(stderr, "the prompts hold %zu tokens, more than the 512 rows of one pass\n", total); return 1; }
            std::vector<std::vector<std::uint32_t>> out(n);
            for (long j = 0; j < n_new; ++j) {
                const std::vector<std::uint32_t> next = batch.forward_runs_sample(runs);
                for (std::uint32_t i = 0; i < n; ++i) {
                    out[i].push_back(next[i]);
                    runs[i].start_pos += static_cast<std::uint32_t>(runs[i].tokens.size());
                    runs[i].tokens.assign(1, next[i]);
                }
            }
            for (std::uint32_t i = 0; i < n; ++i) {
                std::printf("[%u]", i);
                for (std::uint32_t t : out[i]) std::printf(" %u", t);
                std::printf("\n");
            }
            return 0;
        }
        // admission: every prompt but its last token, one run per slot, no outputs - one pass over the weights
        std::vector<lmrs_host::Batch::Run> runs;
        std::vector<std::uint32_t> slot(n), last(n), pos(n);
        std::size_t total = 0;
        for (std::uint32_t i = 0; i < n; ++i) {
            std::vector<std::uint32_t> ids = tok.encode(prompts[i], true, false, false, static_cast<lmrs_host::ModelType>(model.args.model_type));
            if (ids.size() + static_cast<std::size_t>(n_new) - 1 > model.args.seq_len) { std::fprintf(stderr, "prompt %u and %ld tokens exceed seq_len\n", i, n_new); return 1; }
            slot[i] = i; last[i] = ids.back(); pos[i] = static_cast<std::uint32_t>(ids.size() - 1);
            ids.pop_back();
            total += ids.size();
            if (!ids.empty()) runs.push_back(lmrs_host::Batch::Run{i, 0, std::move(ids), 0});
        }
        if (total > 512) { std::fprintf(stderr, "the prompts hold %zu tokens, more than the 512 rows of one pass\n", total); return 1; }
        if (!runs.empty()) batch.forward_runs(runs);
        // one sampler per row: seed + row
        std::vector<std::unique_ptr<lmrs_host::Sampler>> samplers;
        std::vector<lmrs_sampler*> handles;
        for (std::uint32_t i = 0; i < n; ++i) {
            samplers.push_back(std::make_unique<lmrs_host::Sampler>(model.args.vocab_size, temperature, top_p, seed + i));
            handles.push_back(samplers.back()->handle());
        }
        std::vector<std::vector<std::uint32_t>> out(n);
        for (long j = 0; j < n_new; ++j) {
            const std::vector<std::uint32_t> next = batch.forward_sample(slot, last, pos, handles);
            for (std::uint32_t i = 0; i < n; ++i) { out[i].push_back(next[i]); last[i] = next[i]; ++pos[i]; }
        }
        for (std::uint32_t i = 0; i < n; ++i) {
            std::printf("[%u]", i);
            for (std::uint32_t t : out[i]) std::printf(" %u", t);
            std::printf("\n");
        }
    } catch (const lmrs_host::Panic& e) { std::fprintf(stderr, "panic: %s\n", e.what()); return 101; }
    return 0;
}
