// The owner template of lm.rs_amd/csrc/lmrs_buf.h over a counting policy backed by malloc: a stand-alone program (tests/test_buf_host.py builds it
// with -fsanitize=address,undefined where that links).  No HIP is linked; the policy keeps the books the checks read - every block obtained, every
// block released, in order - and can be told to fail the k-th obtain from now.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <utility>
#include <vector>

#include "lmrs_buf.h"

namespace {

struct Counting {
    static std::set<void*> live;                 // obtained and not yet released
    static std::vector<char> log;                // 'o' per obtain that succeeded, 'r' per release
    static size_t obtained, released, last_bytes;
    static long fail_in;                         // > 0: the fail_in-th obtain from now fails
    static void* obtain(size_t bytes) {
        if (fail_in > 0 && --fail_in == 0) return nullptr;
        void* p = malloc(bytes);
        if (!p) abort();
        live.insert(p); log.push_back('o'); ++obtained; last_bytes = bytes;
        return p;
    }
    static void release(void* p) {
        if (!live.erase(p)) { fprintf(stderr, "released a block that is not live (twice, or never obtained)\n"); abort(); }
        free(p); log.push_back('r'); ++released;
    }
};
std::set<void*> Counting::live;
std::vector<char> Counting::log;
size_t Counting::obtained = 0, Counting::released = 0, Counting::last_bytes = 0;
long Counting::fail_in = 0;

template <class T> using CBuf = lmrs::Buf<T, Counting>;

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

void moves() {
    CBuf<float> a;
    CHECK(a.get() == nullptr && a.count() == 0 && !a);
    CHECK(a.alloc(10) && a.count() == 10 && Counting::last_bytes == 40);
    a[9] = 1.0f;                                                   // (the sanitizer watches the block's end)
    float* pa = a;
    CBuf<float> b(std::move(a));
    CHECK(a.get() == nullptr && a.count() == 0);                   // a moved-from owner is empty
    CHECK(b.get() == pa && b.count() == 10);
    CBuf<float> t;
    CHECK(t.alloc(3));
    float* pt = t;
    const size_t rel = Counting::released;
    t = std::move(b);                                              // move-assignment frees the target's old block exactly once
    CHECK(Counting::released == rel + 1 && !Counting::live.count(pt));
    CHECK(t.get() == pa && t.count() == 10 && b.get() == nullptr && b.count() == 0);
    CBuf<float>& same = t;
    t = std::move(same);                                           // (onto itself: nothing moves, nothing is freed)
    CHECK(t.get() == pa && Counting::released == rel + 1);
    std::vector<CBuf<float>> v;                                    // owners in a vector (the transposed scales, the vision tower's blocks): growth moves them
    for (int i = 0; i < 9; ++i) { CBuf<float> e; CHECK(e.alloc((size_t)i)); v.push_back(std::move(e)); }
    CHECK(Counting::live.size() == 1 + 9);
    t.reset();
    CHECK(t.get() == nullptr && t.count() == 0 && Counting::released == rel + 2);
    t.reset();                                                     // (an empty owner releases nothing)
    CHECK(Counting::released == rel + 2);
}

void zero_count() {
    CBuf<double> z;
    const size_t got = Counting::obtained;
    CHECK(z.alloc(0));                                             // a zero count still obtains a block, of 4 bytes
    CHECK(z.get() != nullptr && z.count() == 0 && Counting::obtained == got + 1 && Counting::last_bytes == 4);
}

struct Three { int32_t x[3]; };
void all_or_nothing() {
    const int n = 5;
    for (int k = 1; k <= n + 1; ++k) {                             // the k-th allocation of the set fails (k = n + 1: none does)
        CBuf<float> a; CBuf<char> b; CBuf<Three> c; CBuf<uint64_t> d; CBuf<int> e;
        const size_t got = Counting::obtained, rel = Counting::released, live = Counting::live.size();
        Counting::fail_in = k <= n ? k : 0;
        const bool ok = lmrs::alloc_all({{a, 7}, {b, 0}, {c, 2}, {d, 1}, {e, 100}});
        Counting::fail_in = 0;
        CHECK(ok == (k > n));
        if (!ok) {
            CHECK(!a && !b && !c && !d && !e);                                         // every member is left null,
            CHECK(a.count() == 0 && b.count() == 0 && c.count() == 0 && d.count() == 0 && e.count() == 0);
            CHECK(Counting::obtained == got + (size_t)(k - 1));                         // the members before the k-th were obtained,
            CHECK(Counting::released == rel + (size_t)(k - 1));                         // exactly those were released (twice would have aborted in release),
            CHECK(Counting::live.size() == live);
        } else {
            CHECK(a && b && c && d && e && a.count() == 7 && b.count() == 0 && c.count() == 2 && e.count() == 100);
            CHECK(Counting::obtained == got + (size_t)n && Counting::released == rel);
            c[1].x[2] = 3; e[99] = 1;
        }
    }
}

void regrow() {
    CBuf<float> a; CBuf<char> b;
    CHECK(lmrs::alloc_all({{a, 16}, {b, 16}}));
    const size_t mark = Counting::log.size();
    CHECK(lmrs::alloc_all({{a, 48}, {b, 48}}));                    // the set made anew: the old blocks go before the new ones are obtained
    const std::vector<char> tail(Counting::log.begin() + (long)mark, Counting::log.end());
    CHECK(tail == std::vector<char>({'r', 'r', 'o', 'o'}));
    CHECK(a.count() == 48 && b.count() == 48);
    a[47] = 1.0f; b[47] = 1;
    Counting::fail_in = 2;                                         // a regrow that fails leaves nothing of the old set either
    CHECK(!lmrs::alloc_all({{a, 64}, {b, 64}}));
    Counting::fail_in = 0;
    CHECK(!a && !b);
    CBuf<int> one;                                                 // a lone owner that grows: alloc releases what it held first
    CHECK(one.alloc(4));
    const size_t m2 = Counting::log.size();
    CHECK(one.alloc(8));
    CHECK(Counting::log.size() == m2 + 2 && Counting::log[m2] == 'r' && Counting::log[m2 + 1] == 'o');
    Counting::fail_in = 1;
    CHECK(!one.alloc(16) && !one && one.count() == 0);
    Counting::fail_in = 0;
}

}  // namespace

int main() {
    moves();
    zero_count();
    all_or_nothing();
    regrow();
    CHECK(Counting::live.empty());                                 // at exit, obtained equals released
    CHECK(Counting::obtained == Counting::released && Counting::obtained > 0);
    if (failures) { fprintf(stderr, "buf_check: %d checks failed\n", failures); return 1; }
    printf("buf_check: ok (%zu blocks obtained, %zu released)\n", Counting::obtained, Counting::released);
    return 0;
}
