"""The grow-only buffers (groan_rs_amd/csrc/gr_buf.h) and the worker threads (gr_workers.h) on the CPU: a small C++ driver includes the
headers behind counting stand-ins for hipMalloc / hipFree / hipHostMalloc / hipHostFree, which can be told to fail the n-th allocation.
Pinned here: no allocation while need <= cap, the element count every headroom policy allocates, the state after a failed allocation
(pointer null, capacity 0, the old block freed once, the next call tries again), that the keep-head variant copies exactly the bytes it
was asked to keep, which free call a block goes to, that release() is idempotent, and that at exit every block was freed exactly once.
Of the workers: the thread count rule, that every item is taken exactly once, and that the caller has done the work when no thread could
be started.

The driver is built twice, plainly and with -fsanitize=address,undefined (a stand-alone program, run directly), and every test runs on both.

`pd_out` (the pair-distance output) used to spell its allocation `need ? need : 1` while recording `need`: "allocate 1, record 0".  That
branch was dead -- the block is only ever allocated when need > capacity, which 0 never is -- so what is pinned for it is what the
library did and does: reserve(0) on an empty buffer allocates nothing and leaves pointer null, capacity 0 (test_need_zero...)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "groan_rs_amd", "csrc")

DRIVER = r"""
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <type_traits>
// ---- stand-ins for the four allocation calls: every block is numbered, every call logged
typedef int hipError_t;
static const hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;
static const unsigned hipHostMallocDefault = 0;
struct Block { int id; bool pinned; size_t bytes; int frees; };
static std::map<void *, Block> g_blocks;      // every block ever handed out (the memory itself is freed at the end, so no address comes twice)
static int g_next_id = 1, g_fail_in = 0, g_bad_frees = 0;
static std::string g_log;
static hipError_t fake_alloc(void **p, size_t bytes, bool pinned) {
    if (g_fail_in > 0 && --g_fail_in == 0) { g_log += pinned ? " hostmalloc-FAILED" : " malloc-FAILED"; return hipErrorOutOfMemory; }    // (*p left as it was)
    *p = malloc(bytes ? bytes : 1);
    memset(*p, 0xEE, bytes);
    g_blocks[*p] = Block{ g_next_id, pinned, bytes, 0 };
    g_log += std::string(pinned ? " hostmalloc" : " malloc") + "#" + std::to_string(g_next_id++) + ":" + std::to_string(bytes);
    return hipSuccess;
}
static hipError_t fake_free(void *p, bool pinned) {
    auto it = g_blocks.find(p);
    if (it == g_blocks.end() || it->second.pinned != pinned || it->second.frees) { ++g_bad_frees; g_log += " BAD-FREE"; return 1; }
    it->second.frees = 1;
    g_log += std::string(pinned ? " hostfree" : " free") + "#" + std::to_string(it->second.id);
    return hipSuccess;
}
static hipError_t hipMalloc(void **p, size_t bytes) { return fake_alloc(p, bytes, false); }
static hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return fake_alloc(p, bytes, true); }
static hipError_t hipFree(void *p) { return fake_free(p, false); }
static hipError_t hipHostFree(void *p) { return fake_free(p, true); }
#include "gr_buf.h"
#include "gr_workers.h"

static size_t headroom(const std::string &name, size_t need) {
    if (name == "exact") return grbuf::exact(need);
    if (name == "quarter") return grbuf::quarter(need);
    if (name == "quarter_aligned256") return grbuf::quarter_aligned256(need);
    if (name == "eighth_plus_64") return grbuf::eighth_plus_64(need);
    printf("unknown policy\n"); exit(2);
}
template <class B> static void state(const B &b, hipError_t e, int grew) {
    printf("err %d grew %d ptr %d cap %zu |%s\n", e, grew, b.get() ? 1 : 0, b.cap(), g_log.c_str());
    g_log.clear();
}
static std::atomic<uint32_t> g_deny_from(0xFFFFFFFFu);
static bool may_start(uint32_t t) { return t < g_deny_from.load(); }

int main() {
    {
        grbuf::Dev<uint32_t> dev;                 // 4-byte elements: capacities are elements, allocations bytes
        grbuf::Pinned<unsigned char> pin;
        static_assert(!std::is_copy_constructible<grbuf::Dev<uint32_t>>::value && !std::is_copy_assignable<grbuf::Dev<uint32_t>>::value, "not copyable");
        std::string line;
        while (std::getline(std::cin, line)) {
            std::istringstream in(line);
            std::string op, policy; size_t need = 0;
            in >> op;
            if (op == "fail") { in >> g_fail_in; }
            else if (op == "dev") { in >> policy >> need; bool grew = false; const hipError_t e = dev.reserve(need, [&](size_t n) { return headroom(policy, n); }, &grew); state(dev, e, grew); }
            else if (op == "pin") { in >> policy >> need; bool grew = false; const hipError_t e = pin.reserve(need, [&](size_t n) { return headroom(policy, n); }, &grew); state(pin, e, grew); }
            else if (op == "fill") { for (size_t i = 0; i < pin.cap(); ++i) pin.get()[i] = (unsigned char)(i * 2 + 1); }     // (odd: never the 0xEE of a fresh block)
            else if (op == "keep") {
                size_t k; in >> need >> k;
                const hipError_t e = pin.reserve_keep(need, grbuf::exact, k);
                size_t kept = 0, fresh = 0;
                for (size_t i = 0; i < pin.cap(); ++i) { if (pin.get()[i] == (unsigned char)(i * 2 + 1)) ++kept; else if (pin.get()[i] == 0xEE) ++fresh; }
                printf("kept %zu fresh %zu ", kept, fresh);
                state(pin, e, -1);
            }
            else if (op == "release") { in >> policy; if (policy == "dev") { dev.release(); state(dev, 0, -1); } else { pin.release(); state(pin, 0, -1); } }
            else if (op == "count") { int ht; uint32_t n; in >> ht >> n; printf("%u\n", grw::worker_count(ht, n)); }
            else if (op == "run") {
                // run nt n_items deny_from: every item must be taken once; who worked, and was the work done when start_workers returned?
                uint32_t nt, n_items, deny; in >> nt >> n_items >> deny;
                g_deny_from = deny;
                std::vector<std::atomic<int>> taken(n_items);
                for (auto &t : taken) t.store(0);
                std::atomic<uint32_t> next(0), calls(0), by_caller(0), finished(0);
                const auto me = std::this_thread::get_id();
                std::vector<std::thread> th = grw::start_workers(nt, [&]() {
                    ++calls; if (std::this_thread::get_id() == me) ++by_caller;
                    for (;;) { const uint32_t k = next.fetch_add(1); if (k >= n_items) break; ++taken[k]; }
                    ++finished;
                }, may_start);
                const uint32_t caller_done = by_caller.load() ? finished.load() : 0;      // (the caller's own work is finished before it gets the threads back)
                const size_t handed_back = th.size();
                for (auto &t : th) t.join();
                uint32_t once = 0; for (auto &t : taken) if (t.load() == 1) ++once;
                printf("once %u of %u threads %zu calls %u finished %u by_caller %u caller_done_on_return %u\n", once, n_items, handed_back, calls.load(), finished.load(), by_caller.load(), caller_done);
            }
            else printf("?\n");
            fflush(stdout);
        }
    }   // (the buffers' destructors)
    int live = 0;
    for (auto &kv : g_blocks) { if (kv.second.frees != 1) ++live; free(kv.first); }
    printf("exit: blocks %d not-freed-once %d bad-frees %d |%s\n", g_next_id - 1, live, g_bad_frees, g_log.c_str());
    return 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("buf_" + request.param)
    src, exe = d / "buf_driver.cpp", d / "buf_driver"
    src.write_text(DRIVER)
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-pthread", *flags, "-I" + CSRC, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr

    def run(script):
        """-> the output lines; the last one is the driver's balance at exit and must show every block freed exactly once"""
        r = subprocess.run([str(exe)], input=script + "\n", capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr)      # (a sanitizer report ends the program with a failure)
        out = r.stdout.splitlines()
        assert out[-1].startswith("exit: ") and " not-freed-once 0 bad-frees 0 " in out[-1], out[-1]
        return out
    return run


def test_nothing_is_allocated_while_the_need_fits(driver):
    out = driver("dev exact 100\ndev exact 100\ndev exact 1\ndev exact 0\ndev quarter 100\ndev exact 101")
    assert out[0] == "err 0 grew 1 ptr 1 cap 100 | malloc#1:400"
    assert out[1:5] == ["err 0 grew 0 ptr 1 cap 100 |"] * 4                  # (whatever the policy: it is asked only when the block grows)
    assert out[5] == "err 0 grew 1 ptr 1 cap 101 | free#1 malloc#2:404"      # the old block goes first, its contents are not kept
    assert out[6] == "exit: blocks 2 not-freed-once 0 bad-frees 0 | free#2"  # the destructor frees what is left


def test_need_zero_on_an_empty_buffer_allocates_nothing(driver):
    """(what the pair-distance output does for an empty pair of groups: see the module's docstring)"""
    for policy in ("exact", "quarter", "quarter_aligned256", "eighth_plus_64"):
        out = driver("dev %s 0\npin %s 0" % (policy, policy))
        assert out == ["err 0 grew 0 ptr 0 cap 0 |", "err 0 grew 0 ptr 0 cap 0 |", "exit: blocks 0 not-freed-once 0 bad-frees 0 |"], policy


POLICIES = {"exact": lambda n: n, "quarter": lambda n: n + n // 4, "quarter_aligned256": lambda n: (n + n // 4 + 255) & ~255,
            "eighth_plus_64": lambda n: n + n // 8 + 64}


@pytest.mark.parametrize("policy", sorted(POLICIES))
def test_headroom_policies(driver, policy):
    """capacity = allocation = policy(need), in elements (4 bytes each on the device buffer, 1 on the pinned one)"""
    for need in (1, 3, 4, 8, 255, 256, 1000, 1 << 20):
        want = POLICIES[policy](need)
        out = driver("dev %s %d\npin %s %d" % (policy, need, policy, need))
        assert out[0] == "err 0 grew 1 ptr 1 cap %d | malloc#1:%d" % (want, 4 * want), (need, out)
        assert out[1] == "err 0 grew 1 ptr 1 cap %d | hostmalloc#2:%d" % (want, want), (need, out)
    # the figures themselves, written out once: 1000 elements
    assert {p: f(1000) for p, f in POLICIES.items()} == {"exact": 1000, "quarter": 1250, "quarter_aligned256": 1280, "eighth_plus_64": 1189}
    assert {p: f(1) for p, f in POLICIES.items()} == {"exact": 1, "quarter": 1, "quarter_aligned256": 256, "eighth_plus_64": 65}


def test_failed_allocation_leaves_null_and_zero_and_the_next_call_retries(driver):
    out = driver("dev exact 10\nfail 1\ndev quarter 20\ndev exact 5\ndev exact 5")
    assert out[0] == "err 0 grew 1 ptr 1 cap 10 | malloc#1:40"
    assert out[1] == "err 2 grew 0 ptr 0 cap 0 | free#1 malloc-FAILED"       # the old block freed (once), nothing held
    assert out[2] == "err 0 grew 1 ptr 1 cap 5 | malloc#2:20"                # even a need the old block would have held allocates again
    assert out[3] == "err 0 grew 0 ptr 1 cap 5 |"
    assert out[4] == "exit: blocks 2 not-freed-once 0 bad-frees 0 | free#2"
    # the first allocation of all fails; pinned
    out = driver("fail 1\npin exact 7\npin exact 7")
    assert out[:2] == ["err 2 grew 0 ptr 0 cap 0 | hostmalloc-FAILED", "err 0 grew 1 ptr 1 cap 7 | hostmalloc#1:7"]


def test_keep_head_copies_exactly_the_head(driver):
    # 40 bytes filled with a pattern, grown to 100 keeping 16: bytes 0..15 are the old ones, the other 84 are fresh
    out = driver("pin exact 40\nfill\nkeep 100 16")
    assert out[1] == "kept 16 fresh 84 err 0 grew -1 ptr 1 cap 100 | hostmalloc#2:100 hostfree#1"     # (the new block first: the old one is its source)
    # no old block: nothing to copy
    out = driver("keep 100 16")
    assert out[0] == "kept 0 fresh 100 err 0 grew -1 ptr 1 cap 100 | hostmalloc#1:100"
    # the need fits: no allocation, the block stays as it is
    out = driver("pin exact 40\nfill\nkeep 40 16\nkeep 8 16")
    assert out[1:3] == ["kept 40 fresh 0 err 0 grew -1 ptr 1 cap 40 |"] * 2
    # asked to keep more than the old block holds: its 40 bytes are all there is to copy
    out = driver("pin exact 40\nfill\nkeep 100 64")
    assert out[1] == "kept 40 fresh 60 err 0 grew -1 ptr 1 cap 100 | hostmalloc#2:100 hostfree#1"
    # a failed allocation: null and 0 like reserve(), the old block freed once; the next call allocates again
    out = driver("pin exact 40\nfill\nfail 1\nkeep 100 16\nkeep 100 16")
    assert out[1] == "kept 0 fresh 0 err 2 grew -1 ptr 0 cap 0 | hostmalloc-FAILED hostfree#1"
    assert out[2] == "kept 0 fresh 100 err 0 grew -1 ptr 1 cap 100 | hostmalloc#2:100"


def test_release_is_idempotent_and_picks_the_right_free(driver):
    out = driver("dev exact 3\npin exact 3\nrelease dev\nrelease dev\nrelease pin\nrelease pin\ndev exact 2")
    assert out[2:6] == ["err 0 grew -1 ptr 0 cap 0 | free#1", "err 0 grew -1 ptr 0 cap 0 |", "err 0 grew -1 ptr 0 cap 0 | hostfree#2", "err 0 grew -1 ptr 0 cap 0 |"]
    assert out[6] == "err 0 grew 1 ptr 1 cap 2 | malloc#3:8"                 # usable again afterwards
    assert out[7] == "exit: blocks 3 not-freed-once 0 bad-frees 0 | free#3"


def test_worker_count_is_clamped(driver):
    cases = {(0, 1): 1, (0, 5): 5, (0, 16): 16, (0, 100): 16, (-3, 100): 16, (4, 100): 4, (64, 100): 64, (64, 8): 8, (1, 8): 1, (0, 0): 1, (7, 0): 1}
    out = driver("\n".join("count %d %d" % k for k in cases))
    assert [int(v) for v in out[:-1]] == list(cases.values())


def test_workers_take_every_item_once(driver):
    # run nt n_items deny_from
    out = driver("run 8 1000 99\nrun 3 2 99\nrun 1 50 99")
    assert out[0] == "once 1000 of 1000 threads 8 calls 8 finished 8 by_caller 0 caller_done_on_return 0"
    assert out[1] == "once 2 of 2 threads 3 calls 3 finished 3 by_caller 0 caller_done_on_return 0"
    assert out[2] == "once 50 of 50 threads 1 calls 1 finished 1 by_caller 0 caller_done_on_return 0"      # one thread is started like any other


def test_when_no_thread_starts_the_caller_does_the_work(driver):
    # the start hook refuses every thread: the caller has done all of it when start_workers returns, and gets no thread back
    out = driver("run 8 1000 0\nrun 8 1000 3")
    assert out[0] == "once 1000 of 1000 threads 0 calls 1 finished 1 by_caller 1 caller_done_on_return 1"
    # ... and refuses the fourth: starting stops there, three workers do all of it
    assert out[1] == "once 1000 of 1000 threads 3 calls 3 finished 3 by_caller 0 caller_done_on_return 0"
