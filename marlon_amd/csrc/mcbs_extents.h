// mcbs_extents.h — "no array this call writes may share a byte with another array it reads or writes": the one overlap check of the
// library's entry points (mcbs_api.hip).  Host only, plain C++17, no HIP header: a stand-alone program can compile it.
// (The stride-aware rows_overlap of the logits / GAE gradients is a different check and stays where it is.)
#pragma once

#include <cstddef>
#include <cstdint>

namespace mcbs {

// A fixed-capacity list of byte extents [lo, hi).  An extent is EMPTY — never listed, never overlapping anything — when its pointer is
// null or its rows, width or byte count is 0.  Two listed extents conflict when they intersect and at least one of them is written.
struct Extents {
    // The largest user, the two-agent training turn, lists 72: 4 action arrays, 3 x 5 observation fields, 15 of w, 5 of info, 4 of
    // defender_obs, 13 of dw and 16 of tr.  One more is a programming error, not a caller's: `overflowed`, which the check reports.
    static constexpr size_t kCapacity = 72;
    struct Item { const char* prefix; const char* name; uintptr_t lo, hi; bool written; };     // the message names it prefix + name
    struct Pair { const Item* first; const Item* second; };                                     // first == nullptr: no conflict
    Item item[kCapacity];
    size_t n = 0;
    bool overflowed = false;

    void bytes(const char* name, const void* p, uint64_t n_bytes, bool written, const char* prefix = "") {
        if (!p || !n_bytes) return;
        if (n == kCapacity) { overflowed = true; return; }
        const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
        item[n++] = Item{prefix, name, lo, lo + (uintptr_t)n_bytes, written};
    }
    // `rows` rows `stride` elements of `elem` bytes apart, of which the first `width` elements are used
    void rows(const char* name, const void* p, uint64_t rows, size_t stride, size_t width, size_t elem, bool written) {
        if (rows && width) bytes(name, p, ((rows - 1u) * stride + width) * elem, written);
    }
    // The first conflicting pair in list order, the written array first (both written: in list order)
    Pair overlap() const {
        for (size_t i = 0; i < n; ++i)
            for (size_t k = i + 1u; k < n; ++k)
                if ((item[i].written || item[k].written) && item[i].lo < item[k].hi && item[k].lo < item[i].hi)
                    return item[i].written ? Pair{&item[i], &item[k]} : Pair{&item[k], &item[i]};
        return Pair{nullptr, nullptr};
    }
};

}  // namespace mcbs
