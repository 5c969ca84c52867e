// Who owns a device allocation of the host API (semtsdf_api.cpp).  Host code only, no HIP: the
// includer supplies the raw operations as a type A with
//   static int  A::alloc(void** p, size_t bytes);  // 0, or a status code (*p is then ignored)
//   static void A::free(void* p);
// hipMalloc / hipFree in the library, a counting fake in tests/helpers/own_check.cpp.
//   DevPool<A>      every device allocation of one handle, each recorded with its size: the byte
//                   count is the sum of what is recorded, teardown frees what is left
//   CallScratch<A>  one allocation that lives for one call, freed when its scope ends on every path
#pragma once

#include <cstddef>
#include <initializer_list>
#include <vector>

namespace semtsdf {

template <class A>
class DevPool {
  public:
    struct Req { void** p; size_t bytes; };
    DevPool() = default;
    DevPool(const DevPool&) = delete;
    DevPool& operator=(const DevPool&) = delete;
    ~DevPool() { release_all(); }

    size_t bytes() const { return bytes_; }

    // bytes == 0: a null pointer, and success.  On failure *p is null and nothing is recorded.
    int alloc(void** p, size_t bytes) {
        *p = nullptr;
        if (bytes == 0) return 0;
        if (int rc = A::alloc(p, bytes)) { *p = nullptr; return rc; }
        recs_.push_back({*p, bytes});
        bytes_ += bytes;
        return 0;
    }

    // All of the group or none of it: on failure every pointer of the group is null and nothing
    // of it stays recorded (buffers allocated on first use: "is the first one set" tells for all).
    int alloc_group(std::initializer_list<Req> g) {
        for (const Req& r : g) *r.p = nullptr;
        for (const Req& r : g)
            if (int rc = alloc(r.p, r.bytes)) {
                for (const Req& q : g) { release(*q.p); *q.p = nullptr; }
                return rc;
            }
        return 0;
    }

    // Frees one recorded pointer.  false: the pool does not hold p, and nothing is freed (a null
    // pointer is nobody's and needs no free: true).
    bool release(void* p) {
        if (!p) return true;
        for (size_t i = recs_.size(); i-- > 0;) {
            if (recs_[i].p != p) continue;
            A::free(p);
            bytes_ -= recs_[i].bytes;
            recs_.erase(recs_.begin() + i);
            return true;
        }
        return false;
    }

    // Replaces the owned array *slot by a new one of `bytes`: fill(fresh) writes the new array
    // (0 on success).  Only then is the old one released and *slot set; a failed fill releases
    // the new array and leaves *slot, and the count, as they were.
    template <class Fill>
    int swap(void** slot, size_t bytes, Fill&& fill) {
        void* fresh = nullptr;
        if (int rc = alloc(&fresh, bytes)) return rc;
        if (int rc = fill(fresh)) { release(fresh); return rc; }
        release(*slot);
        *slot = fresh;
        return 0;
    }

    void release_all() { while (!recs_.empty()) release(recs_.back().p); }

  private:
    struct Rec { void* p; size_t bytes; };
    std::vector<Rec> recs_;
    size_t bytes_ = 0;
};

template <class A>
class CallScratch {  // move-only: the move constructor takes the copies away
  public:
    CallScratch() = default;
    CallScratch(CallScratch&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    ~CallScratch() { reset(); }

    // A::alloc's status; what the guard held before is freed first.
    int alloc(size_t bytes) {
        reset();
        const int rc = A::alloc(&p_, bytes);
        if (rc) p_ = nullptr;
        return rc;
    }
    void reset() { if (p_) A::free(p_); p_ = nullptr; }
    template <class T = void> T* get() const { return static_cast<T*>(p_); }

  private:
    void* p_ = nullptr;
};

}  // namespace semtsdf
