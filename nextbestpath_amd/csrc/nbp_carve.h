// nbp_carve.h -- (host) the one way a caller-allocated workspace is cut into buffers.  A workspace's layout is ONE function of a
// Carver and the shape arguments: its *_bytes function runs it dry (no base: only the offset advances) and every launcher runs it
// live on the caller's pointer, so a buffer's size is written once and the size cannot drift from the carve.  Included inside each
// translation unit (anonymous namespace); not part of the C ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace {

struct Carver {
    char* base = nullptr;           // the workspace aligned up to 256; null: a dry run
    size_t off = 0;
    Carver() {}
    explicit Carver(void* ws) : base((char*)round256((uintptr_t)ws)) {}
    static size_t round256(size_t b) { return (b + 255) / 256 * 256; }
    bool dry() const { return !base; }
    // the next buffer, rounded up to the 256-byte alignment of the one after it: its offset from the aligned base
    size_t take_bytes(size_t bytes) { const size_t o = off; off += round256(bytes); return o; }
    template <typename T> T* take(size_t count) {
        const size_t o = take_bytes(count * sizeof(T));
        return base ? (T*)(base + o) : (T*)(uintptr_t)256;      // dry: a non-null dummy, never dereferenced
    }
    size_t end() const { return off; }
    // what the caller must allocate: 256 for aligning the base, the buffers, and the size function's historical slack (kept, by
    // name, because nobody has audited whether a kernel's vector loads run past its last buffer into it)
    size_t bytes(size_t slack = 0) const { return 256 + off + slack; }
};

// A layout function `L layout(Carver&, shape...)` run live on a caller's workspace, and run dry for the bytes that needs.
template <typename F, typename... A> auto carve(const void* ws, F layout, A... shape) { Carver c((void*)ws); return layout(c, shape...); }
template <typename F, typename... A> size_t carved_bytes(size_t slack, F layout, A... shape) { Carver c; layout(c, shape...); return c.bytes(slack); }

}  // namespace
