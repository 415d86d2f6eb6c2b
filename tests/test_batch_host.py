"""The host frame of the batched calls (groan_rs_amd/csrc/gr_batch.h) on the CPU: a small C++ driver includes the header with a fake
context and plays a batched entry point -- per segment the prechecks, then every frame closed, whole or in two sub-ranges -- from a script
of which frames fail where.  Pinned here: the segments of a call, the first error (message, index and counts of the first failing frame in
frame order), that a frame which failed its prechecks is never judged and reports index 0, where status_out is written, that a hard
error ends the walk and is returned as it is, and the rule of the RMSD calls (only one designated status of a segment ends the walk).

The header has no walk function: the call sites write `for (... : grb::Segments{...})` and return a hard error out of that loop
themselves.  So the last two tests pin that IDIOM as the driver writes it -- that Segments stops nothing of its own accord, and that
FirstError::finish is the only place where a noted error is written back; the library's own `if (st) return st;` lines and the
GR_E_HIP rule in rmsd_batch_impl are covered by the GPU suite alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "groan_rs_amd", "csrc")

DRIVER = r"""
#include "gr_batch.h"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
struct Ctx { std::string err = "stale"; uint64_t err_index = 99; uint64_t counts[2] = { 7, 8 }; };
static int fail(Ctx *c, int st, const std::string &msg, uint64_t index = 0) { c->err = msg; c->err_index = index; return st; }
struct Judge { int status; uint64_t idx, c0, c1; };
static void report(const Ctx &c, int ret) { printf("ret %d err '%s' idx %" PRIu64 " counts %" PRIu64 " %" PRIu64 "\n", ret, c.err.c_str(), c.err_index, c.counts[0], c.counts[1]); }
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op; in >> op;
        if (op == "segments") {
            uint32_t n, first; in >> n >> first;
            for (const auto [b0, nb, s0] : grb::Segments{ first, n }) printf("%u %u %u  ", b0, nb, s0);
            printf("\n");
        } else if (op == "call") {
            // call n first with_status split hard_segment hard_status  { p frame status | j frame status idx c0 c1 }...
            uint32_t n, first; int with_status, split, hard_seg, hard_status; in >> n >> first >> with_status >> split >> hard_seg >> hard_status;
            std::map<uint32_t, int> pre_fail; std::map<uint32_t, Judge> judge_fail;
            std::string k;
            while (in >> k) {
                uint32_t f; in >> f;
                if (k == "p") in >> pre_fail[f];
                else { Judge j; in >> j.status >> j.idx >> j.c0 >> j.c1; judge_fail[f] = j; }
            }
            Ctx c;
            std::vector<int> status(n + 2, -7);                       // (one sentinel on either side)
            int *status_out = with_status ? status.data() + 1 : nullptr;
            std::vector<uint32_t> judged;
            grb::FirstError<Ctx> fe;
            int seg_no = 0;
            // (a batched entry point: a hard error returns out of the segment loop, past finish())
            auto entry_point = [&]() -> int {
              for (const grb::Segment seg : grb::Segments{ first, n }) {
                const grb::Prechecks pre(&c, seg, [&](uint32_t slot) {
                    auto it = pre_fail.find(slot - first);
                    return it == pre_fail.end() ? 0 : fail(&c, it->second, "pre, slot " + std::to_string(slot));
                });
                printf("seg %u %u %u all_ok %d any_ok %d\n", seg.b0, seg.nb, seg.s0, pre.all_ok ? 1 : 0, pre.any_ok ? 1 : 0);
                if (seg_no++ == hard_seg) return fail(&c, hard_status, "hard");
                auto close = [&](const grb::PreView &v) {
                    for (uint32_t f = 0; f < v.n; ++f) {
                        const uint32_t frame = v.b0 + f;
                        const int s = grb::close_frame(&c, fe, v, f, status_out, [&]() -> int {
                            judged.push_back(frame);
                            auto it = judge_fail.find(frame);
                            if (it == judge_fail.end()) return 0;
                            c.counts[0] = it->second.c0; c.counts[1] = it->second.c1;
                            return fail(&c, it->second.status, "judge, frame " + std::to_string(frame), it->second.idx);
                        });
                        const int want = pre_fail.count(frame) ? pre_fail[frame] : judge_fail.count(frame) ? judge_fail[frame].status : 0;
                        if (s != want) printf("close_frame returned %d for frame %u\n", s, frame);
                    }
                };
                if (split) {
                    const uint32_t a = seg.nb / 3;
                    const grb::PreView lo = pre.sub(0, a), hi = pre.sub(a, seg.nb);
                    printf("sub %u %u %u all_ok %d any_ok %d | %u %u %u all_ok %d any_ok %d\n", lo.b0, lo.n, lo.s0, lo.all_ok ? 1 : 0, lo.any_ok ? 1 : 0,
                           hi.b0, hi.n, hi.s0, hi.all_ok ? 1 : 0, hi.any_ok ? 1 : 0);
                    close(hi); close(lo);                                // (the later run first: the first error is then the FIRST NOTED, as in the library)
                } else close(pre);
              }
              return fe.finish(&c);
            };
            report(c, entry_point());
            printf("judged %zu", judged.size());
            for (uint32_t f : judged) if (pre_fail.count(f)) printf(" !%u", f);
            printf("\nstatus");
            for (uint32_t f = 0; f < n + 2; ++f) if (status[f] != 0) printf(" %d:%d", (int)f - 1, status[f]);
            printf("\nend\n");
        } else if (op == "rmsd") {
            // rmsd n first designated  status-of-segment...
            uint32_t n, first; int designated; in >> n >> first >> designated;
            std::vector<int> of_segment; int v; while (in >> v) of_segment.push_back(v);
            Ctx c;
            grb::FirstError<Ctx> fe;
            size_t k = 0;
            auto entry_point = [&]() -> int {
              for (const grb::Segment seg : grb::Segments{ first, n }) {
                const int s = k < of_segment.size() ? of_segment[k] : 0;
                ++k;
                if (s) { c.counts[0] = 10 * k; c.counts[1] = 10 * k + 1; (void)fail(&c, s, "segment " + std::to_string(k - 1), seg.b0); }
                if (s == designated) return s;
                fe.note(&c, s);
              }
              return fe.finish(&c);
            };
            report(c, entry_point());
            printf("visited %zu\nend\n", k);
        } else printf("?\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch")
    src, exe = d / "batch_driver.cpp", d / "batch_driver"
    src.write_text(DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + CSRC, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr

    def run(cmd):
        return subprocess.run([str(exe)], input=cmd + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return run


def call(driver, n, first, fails="", with_status=1, split=0, hard_seg=-1, hard_status=0):
    """-> {'seg': [...], 'sub': [...], 'ret': line, 'judged': line, 'status': {frame: status}}"""
    out = driver("call %d %d %d %d %d %d %s" % (n, first, with_status, split, hard_seg, hard_status, fails))
    assert out[-1] == "end" and not [l for l in out if l.startswith("close_frame returned")], out
    res = {"seg": [l for l in out if l.startswith("seg ")], "sub": [l for l in out if l.startswith("sub ")]}
    res["ret"] = [l for l in out if l.startswith("ret ")][0]
    res["judged"] = [l for l in out if l.startswith("judged ")][0]
    res["status"] = {int(t.split(":")[0]): int(t.split(":")[1]) for t in [l for l in out if l.startswith("status")][0].split()[1:]}
    return res


SENTINELS = lambda n: {-1: -7, n: -7}      # the words before and behind status_out stay as they were


def test_segments(driver):
    want = {1: "0 1 3", 1023: "0 1023 3", 1024: "0 1024 3", 1025: "0 1024 3  1024 1 1027", 2048: "0 1024 3  1024 1024 1027",
            2049: "0 1024 3  1024 1024 1027  2048 1 2051"}
    for n, segs in want.items():
        assert driver("segments %d 3" % n) == [segs + "  "], n


def test_no_error_leaves_the_context_alone(driver):
    r = call(driver, 1030, 3)
    assert r["ret"] == "ret 0 err 'stale' idx 99 counts 7 8"
    assert r["seg"] == ["seg 0 1024 3 all_ok 1 any_ok 1", "seg 1024 6 1027 all_ok 1 any_ok 1"]
    assert r["judged"] == "judged 1030" and r["status"] == SENTINELS(1030)


def test_first_error_is_the_first_failing_frame_across_segments(driver):
    # frame 1030 (second segment) fails in its judge, frames 1500 and 2048 (third segment) later with other values
    fails = "j 1030 5 17 100 200 j 1500 6 18 300 400 j 2048 4 19 500 600"
    r = call(driver, 2049, 3, fails)
    assert r["ret"] == "ret 5 err 'judge, frame 1030' idx 17 counts 100 200"
    assert r["status"] == {1030: 5, 1500: 6, 2048: 4, **SENTINELS(2049)}
    # ... and with a failure in the first segment in front of them, that one
    r = call(driver, 2049, 3, "j 1023 9 1 2 3 " + fails)
    assert r["ret"] == "ret 9 err 'judge, frame 1023' idx 1 counts 2 3"
    assert r["status"] == {1023: 9, 1030: 5, 1500: 6, 2048: 4, **SENTINELS(2049)}


def test_a_frame_that_failed_its_prechecks_is_never_judged(driver):
    # the judge would fail frame 1024 as well: it must not be asked
    r = call(driver, 1030, 3, "p 1024 2 j 1024 5 17 1 1 p 1029 3 j 1026 6 44 9 9")
    assert r["judged"] == "judged 1028"                                       # (no "!frame": no judged frame had failed its prechecks)
    assert r["ret"] == "ret 2 err 'pre, slot 1027' idx 0 counts 7 8"          # index 0, the precheck's message, counts untouched
    assert r["status"] == {1024: 2, 1026: 6, 1029: 3, **SENTINELS(1030)}
    assert r["seg"] == ["seg 0 1024 3 all_ok 1 any_ok 1", "seg 1024 6 1027 all_ok 0 any_ok 1"]
    # a segment in which every frame failed them
    r = call(driver, 1026, 0, "p 1024 2 p 1025 2")
    assert r["seg"][1] == "seg 1024 2 1024 all_ok 0 any_ok 0" and r["judged"] == "judged 1024"
    assert r["ret"] == "ret 2 err 'pre, slot 1024' idx 0 counts 7 8"
    # behind a judged failure the precheck's message is restored for the frame, and the first error stays the judged one
    r = call(driver, 10, 0, "j 2 5 17 1 1 p 4 2")
    assert r["ret"] == "ret 5 err 'judge, frame 2' idx 17 counts 1 1" and r["status"] == {2: 5, 4: 2, **SENTINELS(10)}


def test_status_out_offsets_whole_and_in_sub_ranges(driver):
    fails = "p 0 2 j 340 5 17 1 1 j 341 6 18 2 2 j 1023 4 19 3 3 p 1024 3 j 1026 7 20 4 4 j 1029 8 21 5 5"
    want = {0: 2, 340: 5, 341: 6, 1023: 4, 1024: 3, 1026: 7, 1029: 8, **SENTINELS(1030)}
    whole = call(driver, 1030, 3, fails)
    assert whole["status"] == want and whole["ret"] == "ret 2 err 'pre, slot 3' idx 0 counts 7 8"
    # every segment closed as two sub-ranges [0, nb / 3) and [nb / 3, nb), the later one first
    parts = call(driver, 1030, 3, fails, split=1)
    assert parts["status"] == want and parts["judged"] == whole["judged"] == "judged 1028"
    assert parts["sub"] == ["sub 0 341 3 all_ok 0 any_ok 1 | 341 683 344 all_ok 1 any_ok 1", "sub 1024 2 1027 all_ok 0 any_ok 1 | 1026 4 1029 all_ok 1 any_ok 1"]
    assert parts["ret"] == "ret 6 err 'judge, frame 341' idx 18 counts 2 2"      # the first NOTED: frame 341 opens the run that was closed first
    # without status_out: the same call, nothing stored
    for split in (0, 1):
        r = call(driver, 1030, 3, fails, with_status=0, split=split)
        assert r["status"] == {f: -7 for f in range(-1, 1031)} and r["ret"] == (parts if split else whole)["ret"]


def test_a_hard_error_ends_the_walk_and_is_returned_untouched(driver):
    """the idiom of the call sites (the `return` is the driver's own): returning past finish() leaves the noted first error unwritten"""
    # frame 5 fails in the first segment; the second segment's body returns a hard error: the third is never reached
    r = call(driver, 2049, 3, "j 5 5 17 1 1 j 2048 6 18 2 2", hard_seg=1, hard_status=12)
    assert r["seg"] == ["seg 0 1024 3 all_ok 1 any_ok 1", "seg 1024 1024 1027 all_ok 1 any_ok 1"]
    assert r["ret"] == "ret 12 err 'hard' idx 0 counts 1 1"                   # (not frame 5's message and index: nothing was written back)
    assert r["judged"] == "judged 1024" and r["status"] == {5: 5, **{f: -7 for f in range(1024, 2050)}, -1: -7}


def test_the_rmsd_rule_only_the_designated_status_ends_the_walk(driver):
    """the idiom of rmsd_batch_impl (the `if (s == designated) return s;` is the driver's own) over Segments and FirstError::note / finish"""
    def rmsd(n, designated, *of_segment):
        out = driver("rmsd %d 3 %d %s" % (n, designated, " ".join(str(s) for s in of_segment)))
        assert out[-1] == "end"
        return out[0], out[1]
    # other statuses are noted and the walk goes on: the first one is reported, with its own index and counts
    assert rmsd(3000, 12, 0, 5, 6) == ("ret 5 err 'segment 1' idx 1024 counts 20 21", "visited 3")
    # the designated one ends the call where it occurs and is returned as it is, the noted error is not written back
    assert rmsd(3000, 12, 5, 12, 6) == ("ret 12 err 'segment 1' idx 1024 counts 20 21", "visited 2")
    assert rmsd(3000, 12, 12) == ("ret 12 err 'segment 0' idx 0 counts 10 11", "visited 1")
    assert rmsd(3000, 12) == ("ret 0 err 'stale' idx 99 counts 7 8", "visited 3")
