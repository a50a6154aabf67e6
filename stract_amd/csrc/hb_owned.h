// hb_owned.h - the single owners of what the runtime hands out: a device buffer, a block of pinned host words, a stream.
// Include it AFTER hb_guard_alloc.h / hb_pool.h: hipMalloc / hipFree below are then the ones the including file sees (the caching
// allocator, or the debug allocators of hb_guard_alloc.h) - which is also why everything here sits in an unnamed namespace: two
// translation units may see two different pairs.
#pragma once
#include <hip/hip_runtime.h>

namespace {
// The one owner of a hipMalloc'ed buffer.  Move-only; freed when the holder goes out of scope or is assigned over.
template <class T>
struct DevPtr {
    DevPtr() = default;
    explicit DevPtr(T *q) : p(q) {}
    DevPtr(DevPtr &&o) noexcept : p(o.release()) {}
    DevPtr &operator=(DevPtr &&o) noexcept
    {
        reset(o.release());
        return *this;
    }
    DevPtr(const DevPtr &) = delete;
    DevPtr &operator=(const DevPtr &) = delete;
    ~DevPtr() { reset(); }
    T *get() const { return p; }
    explicit operator bool() const { return p != nullptr; }
    T *release()
    {
        T *q = p;
        p = nullptr;
        return q;
    }
    void reset(T *q = nullptr)
    {
        if (p) (void)hipFree(p);
        p = q;
    }
    hipError_t alloc(size_t count) // `count` elements; whatever the holder had is freed first
    {
        reset();
        return hipMalloc((void **)&p, count * sizeof(T));
    }

private:
    T *p = nullptr;
};

// ... of a buffer that only grows: a DevPtr and the entries it was last asked for (`have` means nothing while the holder is empty).
// hold() in hb_api.hip is what allocates it and books its bytes.  Move-only like its base; assigning a fresh one over it frees the buffer
// and forgets the size, which is how a load drops every holder of the graph state.
template <class T>
struct GrowPtr : DevPtr<T> {
    uint64_t have = 0;
};

// ... of hipHostMalloc'ed (pinned) words
template <class T>
struct PinnedPtr {
    PinnedPtr() = default;
    PinnedPtr(const PinnedPtr &) = delete;
    PinnedPtr &operator=(const PinnedPtr &) = delete;
    ~PinnedPtr()
    {
        if (p) (void)hipHostFree(p);
    }
    T *get() const { return p; }
    T &operator[](size_t i) const { return p[i]; }
    hipError_t alloc(size_t count) { return hipHostMalloc((void **)&p, count * sizeof(T)); } // once per holder

private:
    T *p = nullptr;
};

// ... of a non-blocking stream (the device it belongs to must be the current one when the holder dies).  It converts to hipStream_t by
// itself; where a template takes the argument (rocprim::select's predicate overloads) say get() - a copy does not compile.
struct StreamHolder {
    StreamHolder() = default;
    StreamHolder(const StreamHolder &) = delete;
    StreamHolder &operator=(const StreamHolder &) = delete;
    ~StreamHolder()
    {
        if (s) (void)hipStreamDestroy(s);
    }
    hipStream_t get() const { return s; }
    operator hipStream_t() const { return s; }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); } // once per holder

private:
    hipStream_t s = nullptr;
};
} // namespace
