// perplexity.cpp — perplexity of a text under a model (an extension; no reference counterpart): the text is tokenized with BOS
// (Tokenizer::encode, src/tokenizer.rs:66-151), cut into windows of --ctx tokens that start --stride tokens apart, and every window is
// scored from position 0 with Transformer::score (lmrs_score_tokens).  Each token after the first is counted once, in the first window
// that predicts it; nll is the sum of -log p over those tokens, in double, in token order.  Prints one JSON line {"tokens", "nll", "ppl"};
// with --topk K (Transformer::score_topk, lmrs_score_tokens_topk) also "top1" and "topk", the share of counted tokens that were the model's first
// / among its K first candidates, and "mean_rank", the mean number of candidates ahead of the token.
//   usage: perplexity --model m.lmrs --tokenizer tokenizer.bin --text file.txt [--ctx N (default min(seq_len, 512))] [--stride N (default ctx)] [--topk K]
//   g++ -O2 -std=c++17 perplexity.cpp -I../../include -L.. -llmrs_hip -Wl,-rpath,'$ORIGIN/..' -o perplexity
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>

#include "text.hpp"

int main(int argc, char** argv) {
    std::string model_path, tok_path, text_path;
    long ctx_arg = 0, stride_arg = 0, topk = 0;
    for (int i = 1; i + 1 < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--model") model_path = argv[i + 1];
        else if (k == "--tokenizer") tok_path = argv[i + 1];
        else if (k == "--text") text_path = argv[i + 1];
        else if (k == "--ctx") ctx_arg = std::atol(argv[i + 1]);
        else if (k == "--stride") stride_arg = std::atol(argv[i + 1]);
        else if (k == "--topk") { topk = std::atol(argv[i + 1]); if (topk < 1) { std::fprintf(stderr, "--topk needs K >= 1\n"); return 2; } }
        else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (model_path.empty() || tok_path.empty() || text_path.empty()) {
        std::fprintf(stderr, "usage: %s --model m.lmrs --tokenizer tokenizer.bin --text file.txt [--ctx N] [--stride N] [--topk K]\n", argv[0]);
        return 2;
    }
    std::ifstream tf(text_path, std::ios::binary);
    if (!tf) { std::fprintf(stderr, "cannot read %s\n", text_path.c_str()); return 1; }
    const std::string text((std::istreambuf_iterator<char>(tf)), std::istreambuf_iterator<char>());
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
        const std::vector<std::uint32_t> ids = tok.encode(text, true, false, false, static_cast<lmrs_host::ModelType>(model.args.model_type));
        const std::size_t N = ids.size();
        const std::size_t ctx = ctx_arg > 0 ? static_cast<std::size_t>(ctx_arg) : std::min<std::size_t>(model.args.seq_len, 512);
        const std::size_t stride = stride_arg > 0 ? static_cast<std::size_t>(stride_arg) : ctx;
        if (ctx < 2 || ctx > model.args.seq_len || stride > ctx) { std::fprintf(stderr, "need 2 <= ctx <= seq_len and 1 <= stride <= ctx\n"); return 2; }
        if (N < 2) { std::fprintf(stderr, "the text is %zu token(s): nothing to predict\n", N); return 1; }
        double nll = 0.0, rank_sum = 0.0;
        std::size_t counted = 0, done = 1, top1 = 0, topk_hits = 0;        // done: first token not yet predicted
        for (std::size_t b = 0;; b += stride) {
            const std::size_t e = std::min(b + ctx, N);
            if (done < e) {
                const std::vector<std::uint32_t> win(ids.begin() + b, ids.begin() + e);
                const auto s = topk ? model.score_topk(win, static_cast<std::uint32_t>(topk), 0) : lmrs_host::Transformer::ScoreTopk{model.score(win, 0)};
                for (std::size_t j = std::max(b + 1, done); j < e; ++j) {
                    nll -= static_cast<double>(s.logprobs[j - b - 1]); ++counted;
                    if (!topk) continue;
                    const std::uint32_t r = s.target_rank[j - b - 1];
                    top1 += r == 0; topk_hits += r < static_cast<std::uint32_t>(topk); rank_sum += r;
                }
                done = e;
            }
            if (e == N) break;
        }
        std::printf("{\"tokens\": %zu, \"nll\": %.17g, \"ppl\": %.17g", counted, nll, std::exp(nll / static_cast<double>(counted)));
        if (topk) std::printf(", \"k\": %ld, \"top1\": %.6f, \"topk\": %.6f, \"mean_rank\": %.3f", topk, static_cast<double>(top1) / counted,
                              static_cast<double>(topk_hits) / counted, rank_sum / counted);
        std::printf("}\n");
    } catch (const lmrs_host::Panic& e) { std::fprintf(stderr, "panic: %s\n", e.what()); return 101; }
    return 0;
}
