// Page accounting of a paged batch (lmrs_batch_create_paged): per-slot page tables, reference counts, the free list, and the plan-then-commit
// step of every call that writes K/V rows.  Plain C++ with no HIP in it: the device work a call needs comes back as a list of actions ("clear
// page p", "copy page p to q") that lmrs_api.hip enqueues on the context's stream, in order, before the pass.  Page 0 is the zero page: every
// entry starts there, it is never handed out, never counted and never an action's destination.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace lmrs {

struct PageAction { enum Kind : uint32_t { kClear = 0, kCopy = 1 }; uint32_t kind, src, dst; };   // kClear: src is 0
struct PageRange { uint32_t slot, p0, p1; };                                                       // positions [p0, p1) of a slot

class PagePool {
public:
    PagePool(uint32_t n_slots, uint32_t per_slot, uint32_t page_len, uint32_t n_pages);
    // A call that writes the given ranges.  Per page a range touches: an entry of 0 claims a free page (kClear), an entry with more than one holder
    // claims a free page, copies the whole page and drops the old reference (kCopy), an entry this slot holds alone stays.  The plan is computed
    // first: when it wants more pages than are free, false comes back with *wanted set and NOTHING changed.  Otherwise it is committed: the
    // actions are appended to *acts in the order they must run, the slots whose table rows changed to *dirty.
    bool write(const PageRange* ranges, size_t n, std::vector<PageAction>* acts, std::vector<uint32_t>* dirty, uint32_t* wanted);
    // dst's entries of the pages wholly inside [0, n_pos) become references to src's pages (dst's former pages there are dropped); the partial last
    // page, if any, becomes a page dst holds alone - claimed (kClear) or un-shared (kCopy) as in write(), the caller then copies the rows
    // [*part_p0, n_pos) from page *part_src to page *part_dst (equal to 0 / 0 / 0 when there is no partial page).  Fails as write() fails.
    bool fork(uint32_t src, uint32_t dst, uint32_t n_pos, std::vector<PageAction>* acts, std::vector<uint32_t>* dirty, uint32_t* wanted,
              uint32_t* part_p0, uint32_t* part_src, uint32_t* part_dst);
    // keep positions [0, n_pos) of a slot: the entries at index ceil(n_pos / page_len) and above return to 0; a page nobody holds is free
    void release(uint32_t slot, uint32_t n_pos, std::vector<uint32_t>* dirty);

    uint32_t n_slots() const { return n_slots_; }
    uint32_t per_slot() const { return per_slot_; }
    uint32_t page_len() const { return page_len_; }
    uint32_t n_pages() const { return n_pages_; }
    uint32_t n_free() const { return (uint32_t)free_.size(); }
    const uint32_t* row(uint32_t slot) const { return table_.data() + (size_t)slot * per_slot_; }
    uint32_t refs(uint32_t page) const { return refs_[page]; }
    const std::vector<uint32_t>& free_list() const { return free_; }
    void slot_pages(uint32_t slot, uint32_t* held, uint32_t* shared) const;

private:
    uint32_t claim();                       // a free page, one reference
    void drop(uint32_t page);               // one reference less; the last one frees the page
    uint32_t n_slots_, per_slot_, page_len_, n_pages_;
    std::vector<uint32_t> table_, refs_, free_;
};

}  // namespace lmrs
