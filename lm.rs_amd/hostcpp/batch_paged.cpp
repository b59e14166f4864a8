// batch_paged.cpp — a shared-prompt session on a PAGED batch (an extension; no reference counterpart): the --system prompt is tokenized with BOS
// (Tokenizer::encode, src/tokenizer.rs:66-151) and prefilled ONCE into slot 0; every line of --prompts is a continuation of it.  A continuation is
// admitted by forking slot 0 into a free slot - the whole pages of the system prompt are shared, not copied - and feeding its own tokens as a run of
// Batch::forward_runs BESIDE the decode rows of the running continuations; after --n greedy tokens it is printed and its slot released, and the next
// waiting line is admitted into the freed pages.  Up to 63 continuations run at a time (--slots, slot 0 apart); an admission waits while the pool has
// fewer free pages than the continuation can come to need.  Prints the pages held and free at every admission; per line the ids are those of
// batch_greedy on "<system><line>".
//   usage: batch_paged --model m.lmrs --tokenizer tokenizer.bin --system "text" --prompts file.txt [--n N (default 64)] [--slots K (default 8)]
//                      [--page-len L (default 64)] [--pages P (default: what K full sequences would need, halved)]
//   g++ -O2 -std=c++17 batch_paged.cpp -I../../include -L.. -llmrs_hip -Wl,-rpath,'$ORIGIN/..' -o batch_paged
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
    std::string model_path, tok_path, prompts_path, system_text;
    long n_new = 64, n_slots = 8, page_len = 64, n_pages = 0;
    for (int i = 1; i + 1 < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--model") model_path = argv[i + 1];
        else if (k == "--tokenizer") tok_path = argv[i + 1];
        else if (k == "--prompts") prompts_path = argv[i + 1];
        else if (k == "--system") system_text = argv[i + 1];
        else if (k == "--n") n_new = std::atol(argv[i + 1]);
        else if (k == "--slots") n_slots = std::atol(argv[i + 1]);
        else if (k == "--page-len") page_len = std::atol(argv[i + 1]);
        else if (k == "--pages") n_pages = std::atol(argv[i + 1]);
        else { std::fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (model_path.empty() || tok_path.empty() || prompts_path.empty() || system_text.empty() || n_new < 1 || n_slots < 2 || n_slots > 64 || n_pages < 0) {
        std::fprintf(stderr, "usage: %s --model m.lmrs --tokenizer tokenizer.bin --system \"text\" --prompts file.txt [--n N] [--slots 2..64] [--page-len L] [--pages P]\n", argv[0]);
        return 2;
    }
    std::ifstream pf(prompts_path);
    if (!pf) { std::fprintf(stderr, "cannot read %s\n", prompts_path.c_str()); return 1; }
    std::vector<std::string> lines;
    for (std::string line; std::getline(pf, line);) if (!line.empty()) lines.push_back(line);
    if (lines.empty()) { std::fprintf(stderr, "%s holds no prompt\n", prompts_path.c_str()); return 1; }
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
        const auto mt = static_cast<lmrs_host::ModelType>(model.args.model_type);
        const std::uint32_t PL = static_cast<std::uint32_t>(page_len), per_seq = (model.args.seq_len + PL - 1) / PL;
        if (n_pages == 0) n_pages = std::max<long>(per_seq, n_slots * per_seq / 2);
        lmrs_host::Batch batch(model, static_cast<std::uint32_t>(n_slots), PL, static_cast<std::uint32_t>(n_pages));
        const std::vector<std::uint32_t> sys = tok.encode(system_text, true, false, false, mt);
        const std::uint32_t n_sys = static_cast<std::uint32_t>(sys.size());
        batch.prefill(0, sys, 0);                                          // once: every continuation refers to these pages
        const auto form = batch.prefill_form(n_sys, 0);                    // how that call ran: chunks of at most 512 rows, and how many by block attention
        std::printf("system prompt: %u tokens in %u pages of %u positions; %u of %u pages free; prefilled in %u chunk(s), %u by block attention\n", n_sys,
                    batch.slot_pages(0).held, PL, batch.pages().n_free, batch.pages().n_pages, form.n_chunks, form.n_block);
        using Run = lmrs_host::Batch::Run;
        struct Live { std::size_t line; std::vector<std::uint32_t> feed; std::uint32_t pos, last; std::vector<std::uint32_t> out; };     // last: where the continuation ends
        std::vector<Live> slot(static_cast<std::size_t>(n_slots));         // slot[s].feed empty: the slot is free
        std::size_t next_line = 0, done = 0;
        long passes = 0;
        while (done < lines.size()) {
            // admissions: a free slot, a waiting line, and pages for all the continuation can come to write (its own tokens, n_new more, one copied page)
            for (std::uint32_t s = 1; s < n_slots && next_line < lines.size(); ++s) {
                if (!slot[s].feed.empty()) continue;
                std::vector<std::uint32_t> ids = tok.encode(lines[next_line], false, false, false, mt);
                if (ids.empty() || n_sys + ids.size() + static_cast<std::size_t>(n_new) > model.args.seq_len) {
                    std::fprintf(stderr, "line %zu: empty, or too long for seq_len with the system prompt and %ld tokens\n", next_line, n_new); return 1;
                }
                const std::uint32_t need = static_cast<std::uint32_t>((n_sys + ids.size() + n_new + PL - 1) / PL) - n_sys / PL;
                std::uint32_t spoken = 0;                                  // pages the running continuations will still claim
                for (std::uint32_t r = 1; r < n_slots; ++r) if (!slot[r].feed.empty()) spoken += (slot[r].last + PL - 1) / PL - batch.slot_pages(r).held;
                if (batch.pages().n_free < need + spoken) break;           // wait for a running continuation to finish
                batch.fork(0, s, n_sys);
                std::printf("admit line %zu into slot %u: the slot holds %u pages (%u shared); %u of %u pages free\n", next_line, s, batch.slot_pages(s).held,
                            batch.slot_pages(s).shared, batch.pages().n_free, batch.pages().n_pages);
                const std::uint32_t last = n_sys + static_cast<std::uint32_t>(ids.size()) + static_cast<std::uint32_t>(n_new);
                slot[s] = Live{next_line++, std::move(ids), n_sys, last, {}};
            }
            // one pass: every live slot feeds its prompt (first pass after admission) or its last token
            std::vector<Run> runs;
            std::vector<std::uint32_t> who;
            std::size_t rows = 0;
            for (std::uint32_t s = 1; s < n_slots; ++s) {
                if (slot[s].feed.empty() || rows + slot[s].feed.size() > 512) continue;     // (a prompt that does not fit this pass rides in the next)
                rows += slot[s].feed.size();
                runs.push_back(Run{s, slot[s].pos, slot[s].feed, 1});
                who.push_back(s);
            }
            if (runs.empty()) { std::fprintf(stderr, "the pool of %ld pages is too small for one continuation\n", n_pages); return 1; }
            const lmrs_host::Batch::RunsOut o = batch.forward_runs(runs);
            ++passes;
            for (std::size_t j = 0; j < who.size(); ++j) {
                Live& l = slot[who[j]];
                l.pos += static_cast<std::uint32_t>(l.feed.size());
                l.out.push_back(o.argmax[j]);
                l.feed.assign(1, o.argmax[j]);
                if (l.out.size() < static_cast<std::size_t>(n_new)) continue;
                std::string text;
                for (std::uint32_t t : l.out) text += tok.decode(t);
                std::printf("[%zu] %s\n", l.line, text.c_str());
                batch.release(who[j]);                                     // the slot's own pages go back to the pool, the shared ones stay with slot 0
                l = Live{};
                ++done;
            }
        }
        std::printf("%zu continuations x %ld tokens in %ld passes over the weights; %u of %u pages free at the end\n", lines.size(), n_new, passes,
                    batch.pages().n_free, batch.pages().n_pages);
    } catch (const lmrs_host::Panic& e) { std::fprintf(stderr, "panic: %s\n", e.what()); return 101; }
    return 0;
}
