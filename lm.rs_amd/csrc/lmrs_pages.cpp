// Page accounting of a paged batch: see lmrs_pages.h.  No HIP here - tests/pages_fuzz.cpp drives this file on the CPU.
#include "lmrs_pages.h"

#include <algorithm>

namespace lmrs {

PagePool::PagePool(uint32_t n_slots, uint32_t per_slot, uint32_t page_len, uint32_t n_pages)
    : n_slots_(n_slots), per_slot_(per_slot), page_len_(page_len), n_pages_(n_pages), table_((size_t)n_slots * per_slot, 0u), refs_((size_t)n_pages + 1, 0u) {
    free_.reserve(n_pages);
    for (uint32_t p = n_pages; p >= 1; --p) free_.push_back(p);        // a stack: the first claims take pages 1, 2, 3, ..
}

uint32_t PagePool::claim() {
    const uint32_t p = free_.back();
    free_.pop_back();
    refs_[p] = 1;
    return p;
}

void PagePool::drop(uint32_t page) {
    if (page == 0) return;                                             // the zero page is not counted
    if (--refs_[page] == 0) free_.push_back(page);
}

namespace {
struct Step { uint32_t slot, idx, old; };                              // old == 0: claim and clear; else claim, copy `old`, drop it
bool planned(const std::vector<Step>& plan, uint32_t slot, uint32_t idx) {
    return std::any_of(plan.begin(), plan.end(), [&](const Step& s) { return s.slot == slot && s.idx == idx; });
}
void mark(std::vector<uint32_t>* dirty, uint32_t slot) {
    if (dirty && std::find(dirty->begin(), dirty->end(), slot) == dirty->end()) dirty->push_back(slot);
}
}  // namespace

bool PagePool::write(const PageRange* ranges, size_t n, std::vector<PageAction>* acts, std::vector<uint32_t>* dirty, uint32_t* wanted) {
    // the plan: nothing of the pool is written here.  A page two ranges of one call un-share counts its holders as the earlier steps leave them.
    std::vector<Step> plan;
    for (size_t r = 0; r < n; ++r) {
        const PageRange& g = ranges[r];
        if (g.p0 >= g.p1) continue;
        for (uint32_t i = g.p0 / page_len_; i <= (g.p1 - 1) / page_len_; ++i) {
            if (planned(plan, g.slot, i)) continue;
            const uint32_t e = row(g.slot)[i];
            if (e == 0) { plan.push_back(Step{g.slot, i, 0}); continue; }
            const uint32_t leaving = (uint32_t)std::count_if(plan.begin(), plan.end(), [&](const Step& s) { return s.old == e; });
            if (refs_[e] - leaving > 1) plan.push_back(Step{g.slot, i, e});
        }
    }
    if (wanted) *wanted = (uint32_t)plan.size();
    if (plan.size() > free_.size()) return false;
    // the commit
    for (const Step& s : plan) {
        const uint32_t q = claim();
        if (acts) acts->push_back(s.old ? PageAction{PageAction::kCopy, s.old, q} : PageAction{PageAction::kClear, 0, q});
        drop(s.old);                                                   // (never the last reference: the plan saw another holder)
        table_[(size_t)s.slot * per_slot_ + s.idx] = q;
        mark(dirty, s.slot);
    }
    return true;
}

bool PagePool::fork(uint32_t src, uint32_t dst, uint32_t n_pos, std::vector<PageAction>* acts, std::vector<uint32_t>* dirty, uint32_t* wanted,
                    uint32_t* part_p0, uint32_t* part_src, uint32_t* part_dst) {
    const uint32_t full = n_pos / page_len_;
    const bool part = n_pos % page_len_ != 0;
    uint32_t* d = table_.data() + (size_t)dst * per_slot_;
    const uint32_t* s = row(src);
    // the plan: the partial page is the only one that can want a free page (before the full pages' drops: nothing is taken from what this call frees)
    const uint32_t need = part && (d[full] == 0 || refs_[d[full]] > 1) ? 1u : 0u;
    if (wanted) *wanted = need;
    if (need > free_.size()) return false;
    *part_p0 = 0; *part_src = 0; *part_dst = 0;
    if (part) {
        const uint32_t e = d[full];
        if (need) {
            const uint32_t q = claim();
            if (acts) acts->push_back(e ? PageAction{PageAction::kCopy, e, q} : PageAction{PageAction::kClear, 0, q});
            drop(e);
            d[full] = q;
        }
        *part_p0 = full * page_len_; *part_src = s[full]; *part_dst = d[full];
    }
    for (uint32_t i = 0; i < full; ++i) {
        if (d[i] == s[i]) continue;
        if (s[i]) ++refs_[s[i]];
        drop(d[i]);
        d[i] = s[i];
    }
    if (n_pos) mark(dirty, dst);
    return true;
}

void PagePool::release(uint32_t slot, uint32_t n_pos, std::vector<uint32_t>* dirty) {
    uint32_t* t = table_.data() + (size_t)slot * per_slot_;
    for (uint32_t i = (n_pos + page_len_ - 1) / page_len_; i < per_slot_; ++i) {
        if (t[i] == 0) continue;
        drop(t[i]);
        t[i] = 0;
        mark(dirty, slot);
    }
}

void PagePool::slot_pages(uint32_t slot, uint32_t* held, uint32_t* shared) const {
    uint32_t h = 0, sh = 0;
    for (uint32_t i = 0; i < per_slot_; ++i) {
        const uint32_t e = row(slot)[i];
        if (e) { ++h; if (refs_[e] > 1) ++sh; }
    }
    *held = h; *shared = sh;
}

}  // namespace lmrs
