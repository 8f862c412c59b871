// dev_block.h — who owns a block of device memory: one move-only owner per block, and the all-or-nothing ensure of a group of
// them. Plain C++ with no HIP include: the runtime instantiates it over hipMalloc / hipFree (runtime_internal.h: DevBlock), the
// host tests over a counting malloc that fails on request (tests/cpp/dev_block_probe.cpp).
//
// The rules, which every "allocate on first use" and every "grow the table" of the runtime relies on:
//   - a block is a pointer and the element count it was allocated for; the count IS the capacity, nobody keeps a second one;
//   - ensure(n) does nothing when the count is at least n, else frees and allocates n elements; it says whether the pointer
//     moved, so that the caller can drop what baked the old one (a captured graph);
//   - a failed ensure leaves the block EMPTY — pointer null, count 0 — never the old pointer, never a pointer with a count it
//     does not have; a count whose byte size does not fit size_t fails without a call of the allocator;
//   - dev_ensure over several blocks is all or nothing: when one allocation fails every block named is empty afterwards, so
//     no later call finds the group's first member and takes the rest for granted.
// No streams here: a caller that frees a block the device may still be reading waits for its stream first — it knows which.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zgml {

enum class DevEnsure { Failed, Kept, Moved };

// Mem: static void* alloc(size_t bytes) (nullptr: failed) and static void free(void*)
template <class T, class Mem>
class dev_block {
    T* ptr_ = nullptr;
    size_t count_ = 0;

  public:
    dev_block() = default;
    dev_block(const dev_block&) = delete;
    dev_block& operator=(const dev_block&) = delete;
    dev_block(dev_block&& o) noexcept : ptr_(o.ptr_), count_(o.count_) { o.ptr_ = nullptr, o.count_ = 0; }
    dev_block& operator=(dev_block&& o) noexcept {
        if (this != &o) {
            reset();
            ptr_ = o.ptr_, count_ = o.count_;
            o.ptr_ = nullptr, o.count_ = 0;
        }
        return *this;
    }
    ~dev_block() { reset(); }

    operator T*() const { return ptr_; } // (launch arguments and pointer arithmetic read as they do over a raw pointer)
    T* get() const { return ptr_; }
    size_t count() const { return count_; } // elements
    bool holds(size_t n) const { return count_ >= n; }

    void reset() {
        if (ptr_) Mem::free(ptr_);
        ptr_ = nullptr, count_ = 0;
    }

    DevEnsure ensure(size_t n) {
        if (count_ >= n) return DevEnsure::Kept;
        reset();
        if (n > SIZE_MAX / sizeof(T)) return DevEnsure::Failed;
        ptr_ = static_cast<T*>(Mem::alloc(n * sizeof(T)));
        if (!ptr_) return DevEnsure::Failed;
        count_ = n;
        return DevEnsure::Moved;
    }
};

// Groups are named as (block, count) pairs: dev_ensure(a, na, b, nb, ...), element types as they come.
// does every block hold its count already?
inline bool dev_holds() { return true; }
template <class B, class... Rest>
bool dev_holds(const B& b, size_t n, const Rest&... rest) {
    return b.holds(n) && dev_holds(rest...);
}

inline void dev_reset() {}
template <class B, class... Rest>
void dev_reset(B& b, size_t, Rest&... rest) {
    b.reset();
    dev_reset(rest...);
}

inline bool dev_ensure_each(bool*) { return true; }
template <class B, class... Rest>
bool dev_ensure_each(bool* moved, B& b, size_t n, Rest&... rest) {
    const DevEnsure e = b.ensure(n);
    *moved = *moved || e == DevEnsure::Moved;
    return e != DevEnsure::Failed && dev_ensure_each(moved, rest...);
}

// every block to its count, in order, or none: false leaves all of them empty (the ones that held enough before too — whatever
// baked their pointers goes with them, as after a move). `moved`: a pointer is not what it was, also when the call failed
template <class... A>
bool dev_ensure(bool* moved, A&&... a) {
    bool any = false;
    const bool ok = dev_ensure_each(&any, a...);
    if (!ok) dev_reset(a...), any = true;
    if (moved) *moved = any;
    return ok;
}

} // namespace zgml
