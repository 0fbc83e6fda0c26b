// host_threads.h - the one place the library and its programs start worker threads for a loop over indices (host_fmt.h's ordered writer, pm_job.h's
// lanes, oc2pm4's reference-shaped workers and cns_job.h's hand-off are other things and stay where they are).  How many threads is the caller's business:
// every site keeps its own count.  No HIP in this header.
//
// A worker thread does not inherit the caller's thread-local knobs (knobs.h): read knob() before on_threads / deal and capture the value.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

namespace necat_host {

// the machine's hardware threads (at least 1)
inline unsigned hardware_threads() { return std::max(1u, std::thread::hardware_concurrency()); }

// body(tid) on nt threads (tid < nt): nt - 1 are started here, the caller is thread 0; returns when all are done.  What a thread keeps for
// itself (a Worker, buffers) is built inside body.
template <class B>
inline void on_threads(unsigned nt, B&& body)
{
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back([&body, t] { body(t); });
    body(0u);
    for (auto& x : th) x.join();
}

// the indices 0 .. n - 1, handed out in runs of `grain` to whichever thread asks next: run(fn) calls fn(i) until none is left
struct Deal {
    std::atomic<uint64_t> next{0};
    const uint64_t n, grain;
    explicit Deal(uint64_t n_, uint64_t grain_ = 1) : n(n_), grain(std::max<uint64_t>(1, grain_)) {}
    template <class F>
    void run(F&& fn)
    {
        for (;;) {
            const uint64_t b = next.fetch_add(grain);
            if (b >= n) return;
            for (uint64_t i = b; i < std::min(n, b + grain); ++i) fn(i);
        }
    }
};

// fn(i, tid) for every i < n, each exactly once, on nt threads
template <class F>
inline void deal(uint64_t n, unsigned nt, uint64_t grain, F&& fn)
{
    Deal d(n, grain);
    on_threads(nt, [&](unsigned tid) { d.run([&](uint64_t i) { fn(i, tid); }); });
}

}  // namespace necat_host
