// arena_layout.h - how a batch stage lays ONE device allocation out as typed slots.  A stage takes its slots in order from an ArenaLayout, each with the
// element type and count that size it; what it gets back is a Span<T> - a byte offset and that count - and the allocation is bytes() long.  runtime.h binds the
// spans to a DevBuf (ArenaView): the pointer a kernel receives, and the byte count of every copy and fill, then come from the span, not from a second
// expression written beside it.  No HIP in this header (tests/host_core/check_dev_arena.cpp builds it with g++).
#pragma once
#include <stddef.h>

namespace necat {

constexpr size_t kArenaAlign = 256;
inline size_t arena_al(size_t bytes) { return (bytes + (kArenaAlign - 1)) & ~(kArenaAlign - 1); }

// n elements of T at byte `off` of the arena
template <class T>
struct Span {
    size_t off = 0, n = 0;
    size_t bytes() const { return n * sizeof(T); }
    size_t end() const { return off + bytes(); }
};

// The cursor.  Every slot begins at a multiple of 256 bytes and slots do not overlap; take(0) returns the cursor and leaves it where it is (the next slot
// then begins at the same offset: neither has a byte the other could overwrite).
struct ArenaLayout {
    size_t at = 0;
    template <class T> Span<T> take(size_t n) { Span<T> s; s.off = at; s.n = n; at += arena_al(n * sizeof(T)); return s; }
    size_t bytes() const { return at; }
};

}  // namespace necat
