// lmrs_buf.h — owners of memory obtained from the runtime (device and pinned buffers of lmrs_api.hip).
//
// Buf<T, Mem> holds a pointer and an element count, frees in its destructor and moves but never copies.  Mem is a policy with two static
// functions, `void* obtain(size_t bytes)` (null on failure) and `void release(void*)`; nothing of HIP is included here - the two real policies
// stand in lmrs_api.hip, and tests/buf_check.cpp runs the template over a counting malloc policy under the sanitizers.
// The rule: an owner for every block obtained from the runtime, a raw pointer for a view into somebody else's block.
#pragma once
#include <stddef.h>

#include <initializer_list>
#include <utility>

namespace lmrs {

template <class T, class Mem> class Buf {
    T* p_ = nullptr; size_t n_ = 0;
public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
        return *this;
    }
    ~Buf() { reset(); }
    // room for `count` elements, at least 4 bytes (a zero count still obtains a block); what the owner held goes first.  false: it is empty
    bool alloc(size_t count) {
        reset();
        const size_t bytes = count * sizeof(T);
        p_ = static_cast<T*>(Mem::obtain(bytes ? bytes : 4));
        n_ = p_ ? count : 0;
        return p_ != nullptr;
    }
    void reset() { if (p_) Mem::release(p_); p_ = nullptr; n_ = 0; }
    T* get() const { return p_; }
    size_t count() const { return n_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
};

// One member of an all-or-nothing set: an owner of any element type and policy, and the count it is to hold
struct BufWant {
    void* buf; size_t count; bool (*alloc)(void*, size_t); void (*reset)(void*);
    template <class T, class Mem> BufWant(Buf<T, Mem>& b, size_t n)
        : buf(&b), count(n), alloc([](void* q, size_t m) { return static_cast<Buf<T, Mem>*>(q)->alloc(m); }), reset([](void* q) { static_cast<Buf<T, Mem>*>(q)->reset(); }) {}
};
// All or nothing: the whole set is released first (a set that grows is made anew, the old blocks gone before the larger ones are asked for), then its
// members are obtained in order; at the first failure every member is reset and the answer is false - a half-allocated set never reaches a kernel.
inline bool alloc_all(std::initializer_list<BufWant> set) {
    for (const BufWant& w : set) w.reset(w.buf);
    for (const BufWant& w : set)
        if (!w.alloc(w.buf, w.count)) {
            for (const BufWant& u : set) u.reset(u.buf);
            return false;
        }
    return true;
}

}  // namespace lmrs
