// Random write / fork / release operations on lmrs::PagePool (lm.rs_amd/csrc/lmrs_pages.cpp) beside a naive model: per slot, the tag every position
// should read.  The pool's actions are played on a pretend device (one tag per position of every page); after every operation the pool's books
// are audited and every position is read back through the table.  usage: pages_fuzz SEED N_OPS   (exit status 0: every check held)
#include "lmrs_pages.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace lmrs;

static int g_op = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "pages_fuzz: op %d: ", g_op); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

struct Snapshot { std::vector<uint32_t> table, refs, free_list; };
static Snapshot snap(const PagePool& p) {
    Snapshot s;
    for (uint32_t i = 0; i < p.n_slots(); ++i) s.table.insert(s.table.end(), p.row(i), p.row(i) + p.per_slot());
    for (uint32_t q = 0; q <= p.n_pages(); ++q) s.refs.push_back(p.refs(q));
    s.free_list = p.free_list();
    return s;
}
static bool same(const Snapshot& a, const Snapshot& b) { return a.table == b.table && a.refs == b.refs && a.free_list == b.free_list; }

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: pages_fuzz SEED N_OPS\n"); return 2; }
    std::mt19937 rng((uint32_t)std::strtoul(argv[1], nullptr, 10));
    const int n_ops = std::atoi(argv[2]);
    auto pick = [&](uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rng() % (hi - lo + 1)); };          // inclusive
    const uint32_t PL = 1u << pick(1, 3), seq_len = pick(3 * PL, 7 * PL) - pick(0, PL - 1), per_slot = (seq_len + PL - 1) / PL;
    const uint32_t n_slots = pick(2, 7), n_pages = pick(1, n_slots * per_slot);                            // often too few: plans must fail
    PagePool pool(n_slots, per_slot, PL, n_pages);
    std::vector<std::vector<uint64_t>> model(n_slots, std::vector<uint64_t>(seq_len, 0));                  // what every position should read
    std::vector<std::vector<uint64_t>> dev(n_pages + 1, std::vector<uint64_t>(PL, 0));                     // the pretend device: dev[0] is the zero page
    uint64_t tag = 0;
    int failed = 0, forks = 0, copies = 0;

    auto play = [&](const std::vector<PageAction>& acts) {
        for (const PageAction& a : acts) {
            CHECK(a.dst != 0 && a.dst <= n_pages, "an action writes page %u", a.dst);
            CHECK(a.kind == PageAction::kClear || a.src <= n_pages, "an action reads page %u", a.src);
            if (a.kind == PageAction::kClear) dev[a.dst].assign(PL, 0); else { dev[a.dst] = dev[a.src]; ++copies; }
        }
    };
    auto audit = [&]() {
        std::vector<uint32_t> named(n_pages + 1, 0);
        for (uint32_t s = 0; s < n_slots; ++s) for (uint32_t i = 0; i < per_slot; ++i) {
            CHECK(pool.row(s)[i] <= n_pages, "slot %u entry %u names page %u", s, i, pool.row(s)[i]);
            ++named[pool.row(s)[i]];
        }
        uint32_t held = 0;
        for (uint32_t q = 1; q <= n_pages; ++q) {
            CHECK(pool.refs(q) == named[q], "page %u: %u references, %u entries name it", q, pool.refs(q), named[q]);
            held += named[q] != 0;
        }
        CHECK(pool.refs(0) == 0, "the zero page is counted");
        CHECK(held + pool.n_free() == n_pages, "%u held + %u free != %u pages", held, pool.n_free(), n_pages);
        std::vector<char> in_free(n_pages + 1, 0);
        for (uint32_t q : pool.free_list()) {
            CHECK(q >= 1 && q <= n_pages && !in_free[q] && named[q] == 0, "free list: page %u (twice, held or out of range)", q);
            in_free[q] = 1;
        }
        for (uint32_t q = 0; q < PL; ++q) CHECK(dev[0][q] == 0, "the zero page was written");
        for (uint32_t s = 0; s < n_slots; ++s) for (uint32_t p = 0; p < seq_len; ++p)
            CHECK(dev[pool.row(s)[p / PL]][p % PL] == model[s][p], "slot %u position %u reads tag %llu, the model says %llu", s, p,
                  (unsigned long long)dev[pool.row(s)[p / PL]][p % PL], (unsigned long long)model[s][p]);
        for (uint32_t s = 0; s < n_slots; ++s) {
            uint32_t h = 0, sh = 0, mh = 0, msh = 0;
            pool.slot_pages(s, &h, &sh);
            for (uint32_t i = 0; i < per_slot; ++i) if (pool.row(s)[i]) { ++mh; msh += named[pool.row(s)[i]] > 1; }
            CHECK(h == mh && sh == msh, "slot %u: slot_pages says %u held / %u shared, the table %u / %u", s, h, sh, mh, msh);
        }
    };

    for (g_op = 0; g_op < n_ops; ++g_op) {
        const uint32_t what = pick(0, 9);
        const Snapshot before = snap(pool);
        std::vector<PageAction> acts; std::vector<uint32_t> dirty; uint32_t wanted = 0;
        if (what < 5) {                                                  // a call that writes a few ranges: distinct slots as a rule, now and then
            std::vector<PageRange> ranges;                               // any slots - two ranges of one slot may then touch the same page
            std::vector<char> used(n_slots, 0);
            const uint32_t n = pick(1, n_slots < 4 ? n_slots : 4);
            const bool distinct = pick(0, 3) != 0;
            while (ranges.size() < n) {
                const uint32_t s = pick(0, n_slots - 1);
                if (distinct && used[s]) continue;
                used[s] = 1;
                const uint32_t p0 = pick(0, seq_len - 1);
                ranges.push_back(PageRange{s, p0, pick(p0, seq_len)});   // p1 == p0: an empty range
            }
            if (!pool.write(ranges.data(), ranges.size(), &acts, &dirty, &wanted)) {
                CHECK(wanted > before.free_list.size(), "a plan of %u pages failed with %zu free", wanted, before.free_list.size());
                CHECK(acts.empty() && dirty.empty() && same(before, snap(pool)), "a failed write changed the pool");
                ++failed;
            } else {
                CHECK(acts.size() == wanted && before.free_list.size() - pool.n_free() == wanted, "the plan wanted %u pages, %zu actions", wanted, acts.size());
                play(acts);
                for (const PageRange& g : ranges) for (uint32_t p = g.p0; p < g.p1; ++p) {
                    const uint32_t page = pool.row(g.slot)[p / PL];
                    CHECK(page != 0 && pool.refs(page) == 1, "slot %u writes position %u into page %u (%u holders)", g.slot, p, page, pool.refs(page));
                    model[g.slot][p] = dev[page][p % PL] = ++tag;
                }
            }
        } else if (what < 8) {                                           // fork
            const uint32_t src = pick(0, n_slots - 1), dst = (src + pick(1, n_slots - 1)) % n_slots, n_pos = pick(0, seq_len);
            uint32_t p0 = 0, ps = 0, pd = 0;
            if (!pool.fork(src, dst, n_pos, &acts, &dirty, &wanted, &p0, &ps, &pd)) {
                CHECK(wanted > before.free_list.size(), "a fork of %u pages failed with %zu free", wanted, before.free_list.size());
                CHECK(acts.empty() && dirty.empty() && same(before, snap(pool)), "a failed fork changed the pool");
                ++failed;
            } else {
                CHECK(acts.size() <= 1, "a fork costs %zu page actions", acts.size());
                play(acts);
                if (n_pos % PL) {
                    CHECK(pd != 0 && pool.refs(pd) == 1 && pd == pool.row(dst)[n_pos / PL] && ps == pool.row(src)[n_pos / PL] && p0 == n_pos / PL * PL, "fork: the partial page");
                    for (uint32_t p = p0; p < n_pos; ++p) dev[pd][p % PL] = dev[ps][p % PL];
                }
                for (uint32_t p = 0; p < n_pos; ++p) model[dst][p] = model[src][p];
                ++forks;
            }
        } else {                                                         // release
            const uint32_t s = pick(0, n_slots - 1), n_pos = what == 8 ? 0 : pick(0, seq_len);
            pool.release(s, n_pos, &dirty);
            for (uint32_t p = (n_pos + PL - 1) / PL * PL; p < seq_len; ++p) model[s][p] = 0;
            CHECK(pool.n_free() >= before.free_list.size(), "a release took pages");
        }
        audit();
    }
    std::printf("pages_fuzz: %d operations on %u slots x %u entries of %u positions, %u pages: %d refused, %d forks, %d page copies: ok\n", n_ops, n_slots,
                per_slot, PL, n_pages, failed, forks, copies);
    return 0;
}
