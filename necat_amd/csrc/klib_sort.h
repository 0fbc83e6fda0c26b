// klib_sort.h - klib's introsort (klib/ksort.h:180-232) with the same decisions in the same order: median-of-three quicksort on an explicit stack,
// ranges of <= 16 left for one final insertion sort, comb sort when the depth budget runs out.  The sort is unstable, and wherever the reference's
// result depends on the order it leaves equal keys in (the consensus' tag weights, cns_consensus.h; the trimming stage's partition files and chimera
// test, trim_core.h), that permutation is part of the result - so there is one implementation, and both include it.
#pragma once
#include <stddef.h>

#include <vector>

namespace necat_host {

template <class T, class Less>
void klib_insertsort(T* s, T* t, Less lt)
{
    for (T* i = s + 1; i < t; ++i)
        for (T* j = i; j > s && lt(*j, *(j - 1)); --j) { T x = *j; *j = *(j - 1); *(j - 1) = x; }
}

template <class T, class Less>
void klib_combsort(size_t n, T* a, Less lt)
{
    const double shrink = 1.2473309501039786540366528676643;
    size_t gap = n;
    bool swapped;
    do {
        if (gap > 2) { gap = (size_t)(gap / shrink); if (gap == 9 || gap == 10) gap = 11; }
        swapped = false;
        for (T* i = a; i < a + n - gap; ++i) {
            T* j = i + gap;
            if (lt(*j, *i)) { T x = *i; *i = *j; *j = x; swapped = true; }
        }
    } while (swapped || gap > 2);
    if (gap != 1) klib_insertsort(a, a + n, lt);
}

template <class T, class Less>
void klib_introsort(size_t n, T* a, Less lt)
{
    if (n < 1) return;
    if (n == 2) { if (lt(a[1], a[0])) { T x = a[0]; a[0] = a[1]; a[1] = x; } return; }
    int d = 2;
    while ((1ul << d) < n) ++d;
    struct Frame { T* left; T* right; int depth; };
    std::vector<Frame> stack;
    stack.reserve(sizeof(size_t) * d + 2);
    T* s = a; T* t = a + (n - 1);
    d <<= 1;
    for (;;) {
        if (s < t) {
            if (--d == 0) { klib_combsort((size_t)(t - s + 1), s, lt); t = s; continue; }
            T* i = s; T* j = t; T* k = i + ((j - i) >> 1) + 1;
            if (lt(*k, *i)) { if (lt(*k, *j)) k = j; }
            else k = lt(*j, *i) ? i : j;
            const T rp = *k;
            if (k != t) { T x = *k; *k = *t; *t = x; }
            for (;;) {
                do ++i; while (lt(*i, rp));
                do --j; while (i <= j && lt(rp, *j));
                if (j <= i) break;
                T x = *i; *i = *j; *j = x;
            }
            { T x = *i; *i = *t; *t = x; }
            if (i - s > t - i) {
                if (i - s > 16) stack.push_back(Frame{s, i - 1, d});
                s = t - i > 16 ? i + 1 : t;
            } else {
                if (t - i > 16) stack.push_back(Frame{i + 1, t, d});
                t = i - s > 16 ? i - 1 : s;
            }
        } else {
            if (stack.empty()) { klib_insertsort(a, a + n, lt); return; }
            const Frame f = stack.back(); stack.pop_back();
            s = f.left; t = f.right; d = f.depth;
        }
    }
}

}  // namespace necat_host
