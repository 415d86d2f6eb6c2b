// gr_batch.h -- the host frame that every batched entry point shares (no HIP in here: tests/test_batch_host.py drives it with a fake context).
//
// A batched call walks its frames in segments of at most GR_MAX_BATCH (the workspaces are sized for one segment).  Per segment: the
// host checks of every frame (Prechecks), the launches, then every frame is closed (close_frame) -- a frame that failed its checks
// keeps that error and was never touched, any other is judged from what the kernels left.  The call reports every frame's status in
// status_out and returns the FIRST failing frame's status with the message, index and counts that belonged to it (FirstError).  A hard
// error -- a HIP failure, a refused argument -- is none of that: the call returns it at once, out of the segment loop, and writes nothing back.
//
// The context type needs `std::string err; uint64_t err_index; uint64_t counts[2];` and nothing else.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/groan_hip.h"

#define GR_MAX_BATCH 1024    // frames per batched call segment (workspace is sized for this; 82 MB of partial records)

namespace grb {

template <class Ctx>
struct FirstError {
    int first_err = GR_OK;
    std::string msg;
    uint64_t index = 0, counts[2] = { 0, 0 };
    // `s` is a frame's (or a segment's) status and the context's error fields are the ones that came with it
    void note(const Ctx *c, int s) {
        if (s != GR_OK && first_err == GR_OK) { first_err = s; msg = c->err; index = c->err_index; counts[0] = c->counts[0]; counts[1] = c->counts[1]; }
    }
    int finish(Ctx *c) const {
        if (first_err != GR_OK) { c->err = msg; c->err_index = index; c->counts[0] = counts[0]; c->counts[1] = counts[1]; }
        return first_err;
    }
};

struct Segment { uint32_t b0, nb, s0; };    // frames [b0, b0 + nb) of the call, in slots [s0, s0 + nb)

// for (const auto [b0, nb, s0] : grb::Segments{ first_slot, n_frames }): the call's segments in order (the range is its own iterator)
struct Segments {
    uint32_t first_slot, n_frames, b0 = 0;
    Segments begin() const { return *this; }
    int end() const { return 0; }
    bool operator!=(int) const { return b0 < n_frames; }
    void operator++() { b0 += GR_MAX_BATCH; }
    Segment operator*() const { return { b0, std::min<uint32_t>(GR_MAX_BATCH, n_frames - b0), first_slot + b0 }; }
};

// the host checks of `n` consecutive frames: frame f of the view is frame b0 + f of the call and lives in slot s0 + f
struct PreView {
    const int *pre; const std::string *msg;
    uint32_t n, b0, s0;
    bool all_ok = true, any_ok = false;
    PreView(const int *pre_, const std::string *msg_, uint32_t n_, uint32_t b0_, uint32_t s0_) : pre(pre_), msg(msg_), n(n_), b0(b0_), s0(s0_) {
        for (uint32_t f = 0; f < n; ++f) { all_ok = all_ok && pre[f] == GR_OK; any_ok = any_ok || pre[f] == GR_OK; }
    }
    bool ok(uint32_t f) const { return pre[f] == GR_OK; }
    PreView sub(uint32_t a, uint32_t b) const { return PreView(pre + a, msg + a, b - a, b0 + a, s0 + a); }    // frames [a, b) of this view
};

// ... and their owner, one per segment, itself the view of all of it: check(slot) -> GR_OK, or the frame's error with its message in c->err
struct Prechecks : PreView {
    std::vector<int> codes; std::vector<std::string> msgs;
    template <class Ctx, class Check>
    Prechecks(const Ctx *c, const Segment &seg, Check check) : PreView(nullptr, nullptr, 0, 0, 0), codes(seg.nb, GR_OK), msgs(seg.nb) {
        for (uint32_t f = 0; f < seg.nb; ++f) if ((codes[f] = check(seg.s0 + f)) != GR_OK) msgs[f] = c->err;
        static_cast<PreView &>(*this) = PreView(codes.data(), msgs.data(), seg.nb, seg.b0, seg.s0);
    }
    Prechecks(const Prechecks &) = delete;
};

// closes frame f of the view: a frame that failed its checks gets their message back (the index stays what the last fail() left: 0, as
// nothing fails between the checks and here) and is never judged; any other frame's status is judge()'s, which sets the context's error
// fields when it fails.  Noted, stored at status_out[b0 + f] (status_out: the CALL's array, or null), and returned for the caller's own outputs.
template <class Ctx, class Judge>
int close_frame(Ctx *c, FirstError<Ctx> &fe, const PreView &v, uint32_t f, int *status_out, Judge judge) {
    int s = v.pre[f];
    if (s != GR_OK) c->err = v.msg[f];
    else s = judge();
    fe.note(c, s);
    if (status_out) status_out[v.b0 + f] = s;
    return s;
}

}  // namespace grb
