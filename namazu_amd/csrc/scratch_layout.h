// One statement of a scratch buffer's fields. A call lists its fields once, each as the address of a typed
// pointer and an element count (lay.add(&d_off, n_traces + 1)); the layout places them in that order, every field
// rounded up to 256 bytes, and knows the total. bind(buf) asks the buffer for the total once and then stores every
// pointer, so a size and its carving cannot drift apart and element sizes come from the pointers' types alone.
// A zero-count field takes no space and shares the address of the field after it (or the end of the buffer).
// No HIP here: the buffer is any type with ensure(bytes), ptr, and the in-use mark slot / busy (nmz_common.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/nmz_gpu.h"

namespace nmz {

int fail(int code, const std::string &msg);

struct ScratchLayout {
    static constexpr int CAP = 16;
    struct Field {
        void *slot;  // the caller's T *
        void (*set)(void *slot, char *p);
        size_t off;
    };
    Field f[CAP];
    int n = 0;
    size_t total = 0;
    int rc = NMZ_OK;       // the first error of an add(); bind() and place() return it
    bool *held = nullptr;  // the in-use mark of the context slot this layout is bound to

    ScratchLayout() = default;
    ScratchLayout(const ScratchLayout &) = delete;
    ScratchLayout &operator=(const ScratchLayout &) = delete;
    ~ScratchLayout() {
        if (held) *held = false;
    }

    template <typename T>
    ScratchLayout &add(T **p, size_t count) {
        if (rc != NMZ_OK) return *this;
        size_t bytes, end;
        if (n == CAP) {
            rc = fail(NMZ_EINVAL, "scratch layout: more than " + std::to_string(CAP) + " fields");
        } else if (__builtin_mul_overflow(count, sizeof(T), &bytes) || __builtin_add_overflow(bytes, 255, &bytes) ||
                   __builtin_add_overflow(total, bytes & ~size_t(255), &end)) {
            rc = fail(NMZ_ENOMEM, "scratch layout: size overflows size_t");
        } else {
            f[n++] = {p, [](void *s, char *q) { *static_cast<T **>(s) = reinterpret_cast<T *>(q); }, total};
            total = end;
        }
        return *this;
    }
    size_t bytes() const { return total; }
    // store every pointer for a buffer of at least bytes() at base
    int place(void *base) {
        if (rc != NMZ_OK) return rc;
        for (int i = 0; i < n; ++i) f[i].set(f[i].slot, static_cast<char *>(base) + f[i].off);
        return NMZ_OK;
    }
    // A context slot (buf.slot names it) is marked in use until this layout goes out of scope; binding a slot that
    // is marked is a nested reuse, which would free the memory under the outer user's pointers: an error instead.
    template <typename Buf>
    int bind(Buf &buf) {
        if (rc != NMZ_OK) return rc;
        if (buf.slot && buf.busy)
            return fail(NMZ_EINVAL, std::string("scratch slot ") + buf.slot + " is already in use in this call");
        int e = buf.ensure(total);
        if (e != NMZ_OK) return e;
        if (buf.slot) {
            buf.busy = true;
            held = &buf.busy;
        }
        return place(buf.ptr);
    }
};

}  // namespace nmz
