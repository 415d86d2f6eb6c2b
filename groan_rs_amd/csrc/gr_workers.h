// gr_workers.h -- the host worker threads of the xtc reader and writer (no HIP in here: tests/test_buf_host.py drives it).  `work` is a
// loop that takes items off a shared counter until none is left, so any number of threads -- the caller alone included -- finishes the
// job.  A thread that cannot be started must not unwind through the C ABI: starting stops there, and the items it would have taken are
// picked up by the workers that did start, or by the caller.
#pragma once

#include <algorithm>
#include <cstdint>
#include <system_error>
#include <thread>
#include <vector>

namespace grw {

// threads for n_items items: what the caller asked for (host_threads > 0), else one per item up to 16; never more than items, never 0
inline uint32_t worker_count(int host_threads, uint32_t n_items) {
    const uint32_t nt = host_threads > 0 ? (uint32_t)host_threads : std::min<uint32_t>(n_items, 16u);
    return std::max<uint32_t>(1u, std::min<uint32_t>(nt, n_items));
}

// Starts work() on up to nt threads and hands them back for joining; when none could be started, work() has run on the calling thread.
// may_start (tests): thread t is started only if it says so.
template <class Work>
std::vector<std::thread> start_workers(uint32_t nt, Work work, bool (*may_start)(uint32_t) = nullptr) {
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < nt && (!may_start || may_start(t)); ++t) { try { th.emplace_back(work); } catch (const std::system_error &) { break; } }
    if (th.empty()) work();
    return th;
}

}  // namespace grw
