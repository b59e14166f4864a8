// batch_image.cpp — image_prefill.cpp for several images at once: the multimodal prefill of the reference's chat loop (src/bin/chat.rs:84-121) per
// sequence, each into a batch slot of its own, then every sequence's text and the greedy continuation in shared weight passes.
// Per sequence: vision.forward -> processor.forward -> [prefix embeddings | image features | suffix embeddings] -> Batch::prefill_embeddings into
// slot i (ONE fill_kv_cache call of the reference on that slot's cache; the residual rows are not downloaded).  Then ONE Batch::forward_runs admits
// the text tokens of every sequence and returns each one's first new token, and Batch::generate_greedy continues all of them on the device.
// The input of a sequence is what PHI3VProcessor::process would hand on (see image_prefill.cpp): a raw f32 file of num_crops x 576 x 588 normalised
// patch values, and the text after the image as a comma-separated list of token ids.  One line of n_new ids per sequence: what image_prefill prints
// for that image and text alone.
//   usage: batch_image model.lmrs n_new {patches.f32 num_crops w_crop h_crop id,id,...}...
//   g++ -O2 -std=c++17 batch_image.cpp -L.. -llmrs_hip -Wl,-rpath,'$ORIGIN/..' -o batch_image
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "vision.hpp"

int main(int argc, char** argv) {
    if (argc < 8 || (argc - 3) % 5) { std::fprintf(stderr, "usage: %s model.lmrs n_new {patches.f32 num_crops w_crop h_crop id,id,...}...\n", argv[0]); return 2; }
    const int fd = open(argv[1], O_RDONLY);
    if (fd < 0) { std::perror("open"); return 1; }
    struct stat st; fstat(fd, &st);
    const auto* data = static_cast<const std::uint8_t*>(mmap(nullptr, st.st_size, PROT_READ, MAP_PRIVATE, fd, 0));
    if (data == MAP_FAILED) { std::perror("mmap"); return 1; }
    const std::uint32_t n_new = std::atoi(argv[2]), n_seq = (argc - 3) / 5;
    try {
        using namespace lmrs_host;
        auto [model, off_t] = Transformer::create(data, st.st_size);                                        // chat.rs:65
        if (!model.args.multimodal) throw Panic("Cannot use images in a non-multimodal model.");              // :85-88
        auto [vision, off_v] = VisionTransformer::create(data + off_t, st.st_size - off_t);                   // :90
        auto processor = PHI3VProcessor::create(data + off_t + off_v, st.st_size - off_t - off_v);            // :91
        Batch batch(model, n_seq, n_seq > 16);
        std::vector<Batch::Run> text;
        for (std::uint32_t i = 0; i < n_seq; ++i) {
            char** a = argv + 3 + 5 * i;
            const std::uint32_t num_crops = std::atoi(a[1]), w_crop = std::atoi(a[2]), h_crop = std::atoi(a[3]);
            std::vector<float> patches(static_cast<std::size_t>(num_crops) * 576 * 588);
            std::ifstream f(a[0], std::ios::binary);
            if (!f.read(reinterpret_cast<char*>(patches.data()), patches.size() * sizeof(float))) throw Panic("patches file too short");
            auto [patch_embeddings, patch_emb_shape] = vision.forward(patches, num_crops);                    // :106
            const std::vector<float> image_features = processor.forward(patch_embeddings, patch_emb_shape, 336 / 14 / 2, w_crop, h_crop);   // :108
            std::vector<float> rows = model.get_embeddings({1, 32010, 29871, 13});                            // :110
            const std::vector<float> suffix = model.get_embeddings({1, 29871, 13});                           // :112
            rows.insert(rows.end(), image_features.begin(), image_features.end());
            rows.insert(rows.end(), suffix.begin(), suffix.end());
            const std::uint32_t n = static_cast<std::uint32_t>(rows.size() / model.args.dim);
            batch.prefill_embeddings(i, rows, n, 0);                                                          // :119, into slot i
            std::fprintf(stderr, "sequence %u: %zu image embeddings, slot filled to position %u\n", i, image_features.size() / model.args.dim, n);
            std::vector<std::uint32_t> prompt;                                                                // the user's text after the image (:148-187)
            for (char* p = a[4]; *p;) { prompt.push_back(static_cast<std::uint32_t>(std::strtoul(p, &p, 10))); if (*p == ',') ++p; else if (*p) throw Panic("token ids: digits and commas"); }
            if (prompt.empty()) throw Panic("a sequence needs at least one token after its image");
            text.push_back(Batch::Run{i, n, prompt, 1});
        }
        if (!n_new) return 0;
        const std::vector<std::uint32_t> first = batch.forward_runs(text).argmax;                             // every sequence's text in ONE pass
        std::vector<std::uint32_t> slot, pos;
        for (const Batch::Run& r : text) { slot.push_back(r.slot); pos.push_back(r.start_pos + static_cast<std::uint32_t>(r.tokens.size())); }
        const std::vector<std::uint32_t> rest = batch.generate_greedy(slot, first, pos, n_new - 1);           // :188-222 at temperature 0, all sequences a step
        for (std::uint32_t i = 0; i < n_seq; ++i) {
            std::printf("%u ", first[i]);
            for (std::uint32_t j = 0; j + 1 < n_new; ++j) std::printf("%u ", rest[static_cast<std::size_t>(i) * (n_new - 1) + j]);
            std::printf("\n");
        }
    } catch (const lmrs_host::Panic& e) { std::fprintf(stderr, "panic: %s\n", e.what()); return 101; }
    return 0;
}
