// batch_generate.cpp — continuations of several prompts at once from ONE call of the batch's device loop (an extension; no reference counterpart): one
// prompt per line of --prompts (up to 64), each tokenized with BOS (Tokenizer::encode, src/tokenizer.rs:66-151), on a wide batch.  The prompts but their last
// tokens are admitted in ONE call of Batch::forward_runs (lmrs_batch_forward_runs, K/V rows only); then ONE call of Batch::generate (lmrs_batch_generate)
// feeds every prompt's last token and runs every row to the tokenizer's EOS - every row's stop set - or to --n tokens: the stop test, the budget and the
// rows' advance stand on the device, the host looks at the rows' state every --check-every passes and goes on with the live rows alone.  With
// --temperature T > 0 row i samples with Sampler::new(vocab_size, T, 1.0, --seed + i) (sample_mult), else it takes the argmax.  With --top-p P in (0, 1) beside
// it the samplers are the reference's default kind, Sampler::new(vocab_size, T, P, --seed + i), and the call is Batch::generate_topp
// (lmrs_batch_generate_topp: the samplers' candidate vectors live on the device for the length of the call).
// Prints per prompt "[i] (stop|budget, logprob S) text": the finish reason and the sum of the log-probabilities of the tokens it chose.
//   usage: batch_generate --model m.lmrs --tokenizer tokenizer.bin --prompts file.txt [--n N (default 64)] [--check-every K (4)] [--temperature T (0)] [--top-p P (1)] [--seed S (0)]
//   g++ -O2 -std=c++17 batch_generate.cpp -I../../include -L.. -llmrs_hip -Wl,-rpath,'$ORIGIN/..' -o batch_generate
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
    long n_new = 64, check_every = 4;
    float temperature = 0.0f, top_p = 1.0f;
    unsigned long long seed = 0;
    for (int i = 1; i < argc; i += 2) {
        const std::string k = argv[i];
        if (i + 1 >= argc) { std::fprintf(stderr, "option %s needs a value\n", argv[i]); return 2; }
        if (k == "--model") model_path = argv[i + 1];
        else if (k == "--tokenizer") tok_path = argv[i + 1];
        else if (k == "--prompts") prompts_path = argv[i + 1];
        else if (k == "--n") n_new = std::atol(argv[i + 1]);
        else if (k == "--check-every") check_every = std::atol(argv[i + 1]);
        else if (k == "--temperature") temperature = std::strtof(argv[i + 1], nullptr);
        else if (k == "--top-p") top_p = std::strtof(argv[i + 1], nullptr);
        else if (k == "--seed") seed = std::strtoull(argv[i + 1], nullptr, 10);
        else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (model_path.empty() || tok_path.empty() || prompts_path.empty() || n_new < 1 || check_every < 1) {
        std::fprintf(stderr, "usage: %s --model m.lmrs --tokenizer tokenizer.bin --prompts file.txt [--n N] [--check-every K] [--temperature T] [--top-p P] [--seed S]\n", argv[0]);
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
        std::vector<lmrs_host::Batch::Run> admit;                         // every prompt but its last token: K/V rows only
        std::vector<std::uint32_t> slots, last, pos, budget;
        std::vector<std::vector<std::uint32_t>> stop;
        std::vector<std::unique_ptr<lmrs_host::Sampler>> owners;
        std::vector<lmrs_sampler*> samplers;
        std::size_t total = 0;
        for (std::uint32_t i = 0; i < n; ++i) {
            std::vector<std::uint32_t> ids = tok.encode(prompts[i], true, false, false, static_cast<lmrs_host::ModelType>(model.args.model_type));
            if (ids.empty()) { std::fprintf(stderr, "prompt %u holds no token\n", i); return 1; }
            if (ids.size() + static_cast<std::size_t>(n_new) - 1 > model.args.seq_len) { std::fprintf(stderr, "prompt %u and %ld tokens exceed seq_len\n", i, n_new); return 1; }
            slots.push_back(i); last.push_back(ids.back()); pos.push_back(static_cast<std::uint32_t>(ids.size() - 1)); budget.push_back(static_cast<std::uint32_t>(n_new));
            stop.push_back({tok.eos});
            if (temperature > 0.0f) { owners.push_back(std::make_unique<lmrs_host::Sampler>(V, temperature, top_p, seed + i)); samplers.push_back(owners.back()->handle()); }
            ids.pop_back();
            total += ids.size();
            if (!ids.empty()) admit.push_back(lmrs_host::Batch::Run{i, 0, std::move(ids), 0});
        }
        if (total > 512) { std::fprintf(stderr, "the prompts hold %zu tokens, more than the 512 rows of one pass\n", total); return 1; }
        if (!admit.empty()) batch.forward_runs(admit);
        const bool topp = temperature > 0.0f && top_p > 0.0f && top_p < 1.0f;
        const lmrs_host::Batch::Generated g = topp ? batch.generate_topp(slots, last, pos, budget, stop, samplers, static_cast<std::uint32_t>(check_every), /*logprobs=*/true)
                                                   : batch.generate(slots, last, pos, budget, stop, samplers, static_cast<std::uint32_t>(check_every), /*logprobs=*/true);
        for (std::uint32_t i = 0; i < n; ++i) {
            std::string text; double sum = 0.0;
            for (std::size_t j = 0; j < g.tokens[i].size(); ++j) {
                sum += g.logprobs[i][j];
                if (g.tokens[i][j] != tok.eos) text += tok.decode(g.tokens[i][j]);
            }
            std::printf("[%u] (%s, logprob %.4f) %s\n", i, g.finish[i] == lmrs_host::Batch::FINISH_STOP ? "stop" : g.finish[i] == lmrs_host::Batch::FINISH_NO_CANDIDATE ? "no candidate" : "budget", sum, text.c_str());
        }
        std::fprintf(stderr, "%llu passes, %llu row passes, %.3f s\n", static_cast<unsigned long long>(g.passes), static_cast<unsigned long long>(g.row_passes), g.seconds);
    } catch (const lmrs_host::Panic& e) { std::fprintf(stderr, "panic: %s\n", e.what()); return 101; }
    return 0;
}
