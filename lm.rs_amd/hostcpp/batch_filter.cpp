// batch_filter.cpp — sampled continuations of several prompts at once under top-k and min-p truncation (an extension; no reference counterpart): one
// prompt per line of --prompts (up to 64), each tokenized with BOS (Tokenizer::encode, src/tokenizer.rs:66-151), on a wide batch.  The filters are state
// of the slots (Batch::set_filters, lmrs_batch_set_filters, ONE call before the first pass): every sampled row comes from its logits with everything outside
// the --top-k first candidates, and everything whose probability at --temperature is below --min-p times the largest (min_gap = -temperature * ln(min_p),
// Batch::min_p_gap), set to -inf on the device.  So the passes are batch_sample --wide's, unchanged: the whole prompts are admitted in ONE call of
// Batch::forward_runs_sample (lmrs_batch_forward_runs_sample) that also samples each prompt's first token, then every step is one call with runs of one
// token; row i samples with Sampler::new(vocab_size, --temperature, --top-p, --seed + i), on the device.  No logits row crosses to the host.  A row that
// draws EOS stops: its slot leaves the later calls.  Prints "[i] text" per prompt.
//   usage: batch_filter --model m.lmrs --tokenizer tokenizer.bin --prompts file.txt [--n N (default 64)] [--top-k K (40; 0: off)] [--min-p P (0.05; 0: off)]
//                       [--temperature T (0.7)] [--top-p P (0.9)] [--seed S (0)]
//   g++ -O2 -std=c++17 batch_filter.cpp -I../../include -L.. -llmrs_hip -Wl,-rpath,'$ORIGIN/..' -o batch_filter
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
    unsigned long top_k = 40;
    double min_p = 0.05;
    unsigned long long seed = 0;
    for (int i = 1; i < argc; i += 2) {
        const std::string k = argv[i];
        if (i + 1 >= argc) { std::fprintf(stderr, "option %s needs a value\n", argv[i]); return 2; }
        if (k == "--model") model_path = argv[i + 1];
        else if (k == "--tokenizer") tok_path = argv[i + 1];
        else if (k == "--prompts") prompts_path = argv[i + 1];
        else if (k == "--n") n_new = std::atol(argv[i + 1]);
        else if (k == "--top-k") top_k = std::strtoul(argv[i + 1], nullptr, 10);
        else if (k == "--min-p") min_p = std::strtod(argv[i + 1], nullptr);
        else if (k == "--temperature") temperature = std::strtof(argv[i + 1], nullptr);
        else if (k == "--top-p") top_p = std::strtof(argv[i + 1], nullptr);
        else if (k == "--seed") seed = std::strtoull(argv[i + 1], nullptr, 10);
        else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (model_path.empty() || tok_path.empty() || prompts_path.empty() || n_new < 1 || !(min_p >= 0.0 && min_p <= 1.0) || !(temperature >= 0.0f)) {
        std::fprintf(stderr, "usage: %s --model m.lmrs --tokenizer tokenizer.bin --prompts file.txt [--n N] [--top-k K] [--min-p P] [--temperature T] [--top-p P] [--seed S]\n", argv[0]);
        return 2;
    }
    std::ifstream pf(prompts_path);
    if (!pf) { std::fprintf(stderr, "cannot read %s\n", prompts_path.c_str()); return 1; }
    std::vector<std::string> prompts;
    for (std::string line; prompts.size() < 64u && std::getline(pf, line);) if (!line.empty()) prompts.push_back(line);
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
        const std::uint32_t n = static_cast<std::uint32_t>(prompts.size()), V = model.args.vocab_size;
        lmrs_host::Batch batch(model, n, /*wide=*/true);
        // one sampler per prompt (seed + row) and one Filter per slot: min_p in logit space at the samplers' temperature
        const lmrs_host::Batch::Filter filter{static_cast<std::uint32_t>(top_k), lmrs_host::Batch::min_p_gap(min_p, temperature)};
        std::vector<std::unique_ptr<lmrs_host::Sampler>> samplers;
        std::vector<lmrs_host::Batch::SampledRun> runs;
        std::vector<std::uint32_t> row_of, slots;                          // runs[r] is prompt row_of[r]
        std::vector<lmrs_host::Batch::Filter> filters;
        std::size_t total = 0;
        for (std::uint32_t i = 0; i < n; ++i) {
            std::vector<std::uint32_t> ids = tok.encode(prompts[i], true, false, false, static_cast<lmrs_host::ModelType>(model.args.model_type));
            if (ids.size() + static_cast<std::size_t>(n_new) - 1 > model.args.seq_len) { std::fprintf(stderr, "prompt %u and %ld tokens exceed seq_len\n", i, n_new); return 1; }
            total += ids.size();
            slots.push_back(i);
            filters.push_back(filter);
            samplers.push_back(std::make_unique<lmrs_host::Sampler>(V, temperature, top_p, seed + i));
            runs.push_back(lmrs_host::Batch::SampledRun{i, 0, std::move(ids), samplers.back()->handle()});
            row_of.push_back(i);
        }
        if (total > 512) { std::fprintf(stderr, "the prompts hold %zu tokens, more than the 512 rows of one pass\n", total); return 1; }
        batch.set_filters(slots, filters);                                 // state of the slots: every pass below samples from the filtered rows
        std::vector<std::string> text(n);
        for (long j = 0; j < n_new && !runs.empty(); ++j) {
            const std::vector<std::uint32_t> next = batch.forward_runs_sample(runs);
            std::vector<lmrs_host::Batch::SampledRun> go_on;
            std::vector<std::uint32_t> rows;
            for (std::size_t r = 0; r < runs.size(); ++r) {
                const std::uint32_t i = row_of[r];
                if (next[r] == tok.eos) continue;
                text[i] += tok.decode(next[r]);
                lmrs_host::Batch::SampledRun run = runs[r];
                run.start_pos += static_cast<std::uint32_t>(run.tokens.size());
                run.tokens.assign(1, next[r]);
                go_on.push_back(std::move(run)); rows.push_back(i);
            }
            runs = std::move(go_on); row_of = std::move(rows);
        }
        for (std::uint32_t i = 0; i < n; ++i) std::printf("[%u] %s\n", i, text[i].c_str());
    } catch (const lmrs_host::Panic& e) { std::fprintf(stderr, "panic: %s\n", e.what()); return 101; }
    return 0;
}
