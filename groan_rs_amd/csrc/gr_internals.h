// gr_internals.h -- Internals: the value of T atom tuples of one kind (distance, angle, dihedral, cosine against an axis) in every frame of
// a block of resident frames, or their running mean and variance.
//
// The reference has Vector3D::angle and distance only (vector3d.rs:276-278): no dihedral, no per-tuple series; its users download every
// frame and gather in numpy.  DEFINITIONS (include/groan_hip.h has them verbatim): d(a->b) = x_b - x_a, one f32 subtraction per component,
// with GR_IC_PBC followed by gr_min_image_vec with the frame's own box.
//   distance (i, j)         gr_mag3(d(i->j))
//   angle (i, j, k)         u = d(j->i), v = d(j->k): atan2f(|u x v|, u.v)
//   dihedral (i, j, k, l)   b1 = d(i->j), b2 = d(j->k), b3 = d(k->l), n1 = b1 x b2, n2 = b2 x b3: atan2f(|b2| (b1.n2), n1.n2)
//   axis (i, j), a          (d(i->j).a) / |d(i->j)|, 0 when |d| = 0
// Every product and sum of these formulas is rounded on its own (ic_value is compiled with contraction off), so a value's bits do not
// depend on what the kernel does with it afterwards: `accumulate` adds the bits `values` stores.
//   k_fl_check   (gr_series.h, index-list form over the UNIQUE atoms the tuples name) the lowest atom without position, per frame
//   k_ic_walk    <KIND, PBC, ACC>: one wave per workgroup, one tuple per lane.  The tuple table is uint32 [arity][T_pad] on the device, so a
//                wave's index loads are contiguous.  A lane loads its 2 .. 4 atom indices once, turns them into 6 .. 12 byte offsets
//                (gr_tile_index * 4) and walks its frames with the loads of GR_IC_AHEAD frames in flight.  Buffer loads: the frame's slot
//                is the resource, a frame beyond the chunk a resource of zero records, a lane beyond T an offset beyond every slot -- no
//                load carries a condition (gr_layout.h).  The frame's GrBox is read through wave-uniform loads.  blockIdx.x is the range of
//                tuples.
//                ACC = false: blockIdx.y cuts the segment's frames into chunks of frame_chunk frames; the value goes to
//                             out[f * ld + t] (256 contiguous bytes per wave and frame); a failed frame's row is NaN, written by the
//                             same kernel behind a branch on the frame's verdict that is the same in every lane
//                ACC = true:  gridDim.y = 1; the lane keeps o, s, q in registers for the launch, adds its frames in ascending order as
//                             ONE f64 chain and writes the state back; nothing is stored per frame
// THE GATHER is element-granular: 4 B per atom and component, 24 .. 48 B per tuple and frame in 6 .. 12 requests that mostly share cache
// lines (the atoms of a tuple are neighbours in index, and so are the tuples of neighbouring lanes); it leans on L2 and the Infinity Cache.
// GR_IC_AHEAD = 4: the dihedral's 4 x 12 = 48 loads in flight stay below the 63 the hardware's counter of outstanding loads can tell
// apart, and the ring takes 48 registers.
// WORKSPACE of gr_internals_values_batch (host): the device variant runs into a grow-only [frames][T_pad] buffer of at most
// GR_IC_MAX_WS_BYTES; where T_pad x 1024 x 4 B is more, the segment is walked in pieces of fewer frames.  No result depends on the piece.
#pragma once
#include "gr_fluct.h"

#if defined(__HIPCC__)

#define GR_IC_AHEAD 4                     /* frames whose loads a lane has in flight */
#define GR_IC_WG 64u                      /* lanes of a workgroup of k_ic_walk: one wave */
#define GR_IC_MAX_RANGES (1u << 22)       /* k_ic_walk's grid along x at most */
#define GR_IC_FILL_WAVES 2048u            /* waves a launch aims at: 8 per compute unit of a 256-unit device */

struct GrIcState {
    float *o;                             // [T_pad]
    double *s, *q;
};

struct gr_internals {
    gr_ctx *c = nullptr;
    int kind = 0;
    uint32_t flags = 0, arity = 0, T = 0, tpad = 0;
    float axis[3] = { 0.0f, 0.0f, 0.0f };
    GrTuples tab;                         // the tuples, the atoms they name, the device table [arity][T_pad]
    GrVerdicts verdicts;
    grbuf::Dev<float> o, ws;              // [T_pad]; values_batch's workspace
    grbuf::Dev<double> s, q;              // [T_pad]
    uint64_t n = 0;                       // frames counted by accumulate
    uint32_t tuple_ranges = 0, frame_chunk = 0;       // gr_internals_set_launch; 0: the default
    uint32_t last_wx = 0, last_wy = 0, last_check = 0;
    uint64_t launches = 0;
};

namespace {

constexpr int ic_arity(int kind) { return kind == GR_IC_ANGLE ? 3 : (kind == GR_IC_DIHEDRAL ? 4 : 2); }

// the value of one tuple from the positions of its atoms, p[3 * a + c]
template <int KIND, bool PBC>
__device__ __forceinline__ float ic_value(const float (&p)[3 * ic_arity(KIND)], const GrBox &box, float ax, float ay, float az) {
#pragma clang fp contract(off)
    auto disp = [&](int a, int b, float &dx, float &dy, float &dz) {
        dx = p[3 * b] - p[3 * a]; dy = p[3 * b + 1] - p[3 * a + 1]; dz = p[3 * b + 2] - p[3 * a + 2];
        if (PBC) gr_min_image_vec(dx, dy, dz, box);
    };
    if (KIND == GR_IC_DISTANCE) {
        float dx, dy, dz;
        disp(0, 1, dx, dy, dz);
        return gr_mag3(dx, dy, dz);
    } else if (KIND == GR_IC_AXIS) {
        float dx, dy, dz;
        disp(0, 1, dx, dy, dz);
        const float len = gr_mag3(dx, dy, dz);
        const float dot = dx * ax + dy * ay + dz * az;
        return len > 0.0f ? dot / len : 0.0f;
    } else if (KIND == GR_IC_ANGLE) {
        float ux, uy, uz, vx, vy, vz;
        disp(1, 0, ux, uy, uz);
        disp(1, 2, vx, vy, vz);
        const float cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
        return atan2f(gr_mag3(cx, cy, cz), ux * vx + uy * vy + uz * vz);
    } else {
        float b1x, b1y, b1z, b2x, b2y, b2z, b3x, b3y, b3z;
        disp(0, 1, b1x, b1y, b1z);
        disp(1, 2, b2x, b2y, b2z);
        disp(2, 3, b3x, b3y, b3z);
        const float n1x = b1y * b2z - b1z * b2y, n1y = b1z * b2x - b1x * b2z, n1z = b1x * b2y - b1y * b2x;
        const float n2x = b2y * b3z - b2z * b3y, n2y = b2z * b3x - b2x * b3z, n2z = b2x * b3y - b2y * b3x;
        const float y = gr_mag3(b2x, b2y, b2z) * (b1x * n2x + b1y * n2y + b1z * n2z);
        return atan2f(y, n1x * n2x + n1y * n2y + n1z * n2z);
    }
}

// d = v - o as the sums take it: ONE f32 subtraction, for a dihedral reduced once into [-PI_F, PI_F]
template <int KIND>
__device__ __forceinline__ float ic_delta(float v, float o) {
#pragma clang fp contract(off)
    float d = v - o;
    if (KIND == GR_IC_DIHEDRAL) {
        const float PI_F = (float)M_PI;
        if (d > PI_F) d -= 2.0f * PI_F;
        else if (d < -PI_F) d += 2.0f * PI_F;
    }
    return d;
}

// frames [s0, s0 + nf) of `frames`; verdict[f] per frame, readable up to verdict[nf + 2 * GR_IC_AHEAD); table: [arity][tpad]
// ACC = false: out points at the row of frame 0, rows are ld floats apart; gridDim.y * frame_chunk >= nf
// ACC = true:  S is the state, have_origin: the object has counted a frame before this launch
template <int KIND, bool PBC, bool ACC>
__global__ __launch_bounds__(GR_IC_WG) void k_ic_walk(const float *__restrict__ frames, size_t stride, uint32_t slot_bytes, uint32_t s0, uint32_t nf,
                                                      const uint32_t *__restrict__ table, uint32_t T, uint32_t tpad, const GrBox *__restrict__ boxes,
                                                      const uint32_t *__restrict__ verdict, float ax, float ay, float az, uint32_t frame_chunk,
                                                      float *__restrict__ out, size_t ld, GrIcState S, uint32_t have_origin) {
    constexpr int A = ic_arity(KIND), C = 3 * A;
    const uint32_t per = (T + gridDim.x - 1u) / gridDim.x;
    const uint32_t t0 = (uint32_t)min((uint64_t)blockIdx.x * per, (uint64_t)T), t1 = (uint32_t)min((uint64_t)t0 + per, (uint64_t)T);
    // the workgroup's frames
    const uint32_t f0 = ACC ? 0u : (uint32_t)min((uint64_t)blockIdx.y * frame_chunk, (uint64_t)nf);
    const uint32_t f1 = ACC ? nf : (uint32_t)min((uint64_t)f0 + frame_chunk, (uint64_t)nf);
    if (f0 >= f1) return;
    // the frame's slot as a buffer: zero records beyond the chunk (and then the last frame's address, so that nothing points outside the slots)
    auto slot_of = [&](uint32_t f) {
        return gr_buf_rsrc(frames + (size_t)(s0 + min(f, f1 - 1u)) * stride, f < f1 ? slot_bytes : 0u);
    };
    const float qnan = __uint_as_float(0x7fc00000u);
    for (uint32_t tb = t0; tb < t1; tb += GR_IC_WG) {
        const uint32_t t = tb + threadIdx.x;
        const bool live = t < t1;
        uint32_t off[C];
#pragma unroll
        for (int j = 0; j < C; ++j) off[j] = GR_BUF_NOWHERE;
        if (live) {
#pragma unroll
            for (int a = 0; a < A; ++a) {
                const uint32_t i = table[(size_t)a * tpad + t];
#pragma unroll
                for (int c = 0; c < 3; ++c) off[3 * a + c] = (uint32_t)gr_tile_index(i, c) * 4u;
            }
        }
        auto request = [&](uint32_t f, float (&v)[C]) {
            const __amdgpu_buffer_rsrc_t rs = slot_of(f);
#pragma unroll
            for (int j = 0; j < C; ++j) v[j] = gr_buf_load_f32(rs, off[j]);
        };
        // the tuple's state, requested before the first positions (loads return in order)
        float o = 0.0f;
        double s = 0.0, q = 0.0;
        if (ACC && live) { o = S.o[t]; s = S.s[t]; q = S.q[t]; }
        float ring[GR_IC_AHEAD][C];
#pragma unroll
        for (int k = 0; k < GR_IC_AHEAD; ++k) {
            request(f0 + (uint32_t)k, ring[k]);
            __builtin_amdgcn_sched_barrier(0);      // in frame order (k_fl_accumulate)
        }
        bool have = have_origin != 0u;
        // the verdicts of a turn of the ring are requested one turn ahead (k_fl_accumulate)
        uint32_t vnext[GR_IC_AHEAD];
#pragma unroll
        for (int k = 0; k < GR_IC_AHEAD; ++k) vnext[k] = verdict[f0 + (uint32_t)k];
        for (uint32_t base = f0; base < f1; base += GR_IC_AHEAD) {
            uint32_t vcur[GR_IC_AHEAD];
#pragma unroll
            for (int k = 0; k < GR_IC_AHEAD; ++k) { vcur[k] = vnext[k]; vnext[k] = verdict[base + GR_IC_AHEAD + (uint32_t)k]; }
#pragma unroll
            for (int k = 0; k < GR_IC_AHEAD; ++k) {
                const uint32_t f = base + (uint32_t)k;
                if (f < f1) {                                       // (the same in every lane, as is the branch on the verdict)
                    if (vcur[k] == GR_NOIDX) {
                        const float v = ic_value<KIND, PBC>(ring[k], boxes[s0 + f], ax, ay, az);
                        if (ACC) {
                            if (!have) { o = v; have = true; }
                            const double dd = (double)ic_delta<KIND>(v, o);
                            s += dd;
                            q = fma(dd, dd, q);
                        } else if (live) {
                            out[(size_t)f * ld + t] = v;
                        }
                    } else if (!ACC && live) {
                        out[(size_t)f * ld + t] = qnan;
                    }
                }
                request(f + GR_IC_AHEAD, ring[k]);                  // behind the frame's work: into the registers it has just left
            }
        }
        if (ACC && live) { S.o[t] = o; S.s[t] = s; S.q[t] = q; }
    }
}

typedef void (*ic_kernel_t)(const float *, size_t, uint32_t, uint32_t, uint32_t, const uint32_t *, uint32_t, uint32_t, const GrBox *, const uint32_t *, float, float,
                            float, uint32_t, float *, size_t, GrIcState, uint32_t);

template <bool ACC>
ic_kernel_t ic_kernel(int kind, bool pbc) {
    switch (kind) {
    case GR_IC_DISTANCE: return pbc ? k_ic_walk<GR_IC_DISTANCE, true, ACC> : k_ic_walk<GR_IC_DISTANCE, false, ACC>;
    case GR_IC_ANGLE: return pbc ? k_ic_walk<GR_IC_ANGLE, true, ACC> : k_ic_walk<GR_IC_ANGLE, false, ACC>;
    case GR_IC_DIHEDRAL: return pbc ? k_ic_walk<GR_IC_DIHEDRAL, true, ACC> : k_ic_walk<GR_IC_DIHEDRAL, false, ACC>;
    default: return pbc ? k_ic_walk<GR_IC_AXIS, true, ACC> : k_ic_walk<GR_IC_AXIS, false, ACC>;
    }
}

int ic_get(gr_internals *ic, std::vector<float> &o, std::vector<double> &s, std::vector<double> &q) {
    gr_ctx *c = ic->c;
    (void)hipSetDevice(c->device);
    o.resize(ic->T); s.resize(ic->T); q.resize(ic->T);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(o.data(), ic->o.get(), ic->T * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(s.data(), ic->s.get(), ic->T * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(q.data(), ic->q.get(), ic->T * sizeof(double), hipMemcpyDeviceToHost));
    return GR_OK;
}

int ic_put(gr_internals *ic, const std::vector<float> &o, const std::vector<double> &s, const std::vector<double> &q) {
    gr_ctx *c = ic->c;
    (void)hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(ic->o.get(), o.data(), ic->T * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(ic->s.get(), s.data(), ic->T * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(ic->q.get(), q.data(), ic->T * sizeof(double), hipMemcpyHostToDevice));
    return GR_OK;
}

int ic_zero(gr_internals *ic) {
    gr_ctx *c = ic->c;
    HIPCHK(c, hipMemsetAsync(ic->o.get(), 0, ic->tpad * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(ic->s.get(), 0, ic->tpad * sizeof(double), c->stream));
    HIPCHK(c, hipMemsetAsync(ic->q.get(), 0, ic->tpad * sizeof(double), c->stream));
    ic->n = 0;
    return GR_OK;
}

// x brought into (-pi, pi]
double ic_wrap_pi(double x) {
    while (x > M_PI) x -= 2.0 * M_PI;
    while (x <= -M_PI) x += 2.0 * M_PI;
    return x;
}

uint32_t ic_ranges(const gr_internals *ic) {
    return std::min<uint32_t>(ic->tuple_ranges ? ic->tuple_ranges : (ic->T + GR_IC_WG - 1u) / GR_IC_WG, GR_IC_MAX_RANGES);
}

// the frames of one workgroup of a `values` launch over nf frames.  The default: T alone gives wx waves; where that is fewer than
// GR_IC_FILL_WAVES the frames are cut so that wx * wy reaches it -- but a chunk keeps at least 2 * GR_IC_AHEAD frames, so that the
// prologue (index loads, offsets, the first ring of requests) stays a small part of a workgroup's work.
uint32_t ic_chunk(const gr_internals *ic, uint32_t wx, uint32_t nf) {
    if (ic->frame_chunk) return std::min(ic->frame_chunk, nf);
    const uint32_t want = (GR_IC_FILL_WAVES + wx - 1u) / wx;
    const uint32_t most = std::max<uint32_t>(1u, nf / (2u * GR_IC_AHEAD));
    const uint32_t wy = std::min(want, most);
    return (nf + wy - 1u) / wy;
}

// out_dev (rows ld floats apart) or out_host ([n_frames][T]); exactly one of them
int ic_values(gr_internals *ic, uint32_t first_slot, uint32_t n_frames, float *out_host, float *out_dev, uint64_t ld, int *status_out) {
    gr_ctx *c = ic->c;
    int st = slot_check(c, first_slot, n_frames); if (st) return st;
    (void)hipSetDevice(c->device);
    const bool pbc = (ic->flags & GR_IC_PBC) != 0u;
    const uint32_t slot_bytes = (uint32_t)(c->frame_stride * sizeof(float));
    const GrIcState none = { nullptr, nullptr, nullptr };
    const ic_kernel_t kernel = ic_kernel<false>(ic->kind, pbc);
    GrVerdicts &V = ic->verdicts;
    const uint32_t *vd = V.dev.get();
    // host variant: frames per piece of the workspace
    const uint32_t piece = (uint32_t)std::max<size_t>(1u, std::min<size_t>(GR_MAX_BATCH, GR_IC_MAX_WS_BYTES / ((size_t)ic->tpad * sizeof(float))));
    if (out_host && ic->ws.reserve((size_t)std::min(piece, n_frames) * ic->tpad, grbuf::exact) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, GR_E_HIP, "internals: device allocation failed");
    }
    grb::FirstError<gr_ctx> fe;
    for (const auto [b0, nb, s0] : grb::Segments{ first_slot, n_frames }) {
        const grb::Prechecks pre(c, { b0, nb, s0 }, box_checks(c, pbc));
        {
            SlotUse use(c, s0, nb);
            st = V.begin(c, pre, nb); if (st) return st;
            ic->last_check = V.check(c, ic->tab.uniq, s0, nb);
            const uint32_t wx = ic_ranges(ic);
            for (uint32_t p0 = 0; p0 < nb; p0 += out_host ? piece : nb) {
                const uint32_t np = out_host ? std::min(piece, nb - p0) : nb;
                const uint32_t chunk = ic_chunk(ic, wx, np), wy = (np + chunk - 1u) / chunk;
                float *rows = out_host ? ic->ws.get() : out_dev + (size_t)b0 * ld;
                const size_t row_ld = out_host ? ic->tpad : (size_t)ld;
                kernel<<<dim3(wx, wy), dim3(GR_IC_WG), 0, c->stream>>>(c->frames, c->frame_stride, slot_bytes, s0 + p0, np, ic->tab.table_dev.get(), ic->T, ic->tpad,
                                                                       c->boxes_dev, vd + p0, ic->axis[0], ic->axis[1], ic->axis[2], chunk, rows, row_ld, none, 0u);
                HIPCHK(c, hipGetLastError());
                ++ic->launches; ic->last_wx = wx; ic->last_wy = wy;
                if (out_host) {
                    HIPCHK(c, hipStreamSynchronize(c->stream));
                    HIPCHK(c, hipMemcpy2D(out_host + (size_t)(b0 + p0) * ic->T, ic->T * sizeof(float), rows, row_ld * sizeof(float), ic->T * sizeof(float), np, hipMemcpyDeviceToHost));
                }
            }
            st = V.end(c, nb); if (st) return st;
        }
        for (uint32_t k = 0; k < nb; ++k) grb::close_frame(c, fe, pre, k, status_out, [&] { return V.judge(c, k); });
    }
    return fe.finish(c);
}

int ic_accumulate(gr_internals *ic, uint32_t first_slot, uint32_t n_frames, int *status_out) {
    gr_ctx *c = ic->c;
    int st = slot_check(c, first_slot, n_frames); if (st) return st;
    (void)hipSetDevice(c->device);
    const bool pbc = (ic->flags & GR_IC_PBC) != 0u;
    const uint32_t slot_bytes = (uint32_t)(c->frame_stride * sizeof(float));
    const GrIcState S = { ic->o.get(), ic->s.get(), ic->q.get() };
    const ic_kernel_t kernel = ic_kernel<true>(ic->kind, pbc);
    GrVerdicts &V = ic->verdicts;
    const uint32_t *vd = V.dev.get();
    grb::FirstError<gr_ctx> fe;
    for (const auto [b0, nb, s0] : grb::Segments{ first_slot, n_frames }) {
        const grb::Prechecks pre(c, { b0, nb, s0 }, box_checks(c, pbc));
        if (pre.any_ok) {
            SlotUse use(c, s0, nb);
            st = V.begin(c, pre, nb); if (st) return st;
            ic->last_check = V.check(c, ic->tab.uniq, s0, nb);
            const uint32_t wx = ic_ranges(ic);
            kernel<<<dim3(wx), dim3(GR_IC_WG), 0, c->stream>>>(c->frames, c->frame_stride, slot_bytes, s0, nb, ic->tab.table_dev.get(), ic->T, ic->tpad, c->boxes_dev, vd,
                                                               ic->axis[0], ic->axis[1], ic->axis[2], nb, nullptr, 0, S, ic->n ? 1u : 0u);
            HIPCHK(c, hipGetLastError());
            ++ic->launches; ic->last_wx = wx; ic->last_wy = 1u;
            st = V.end(c, nb); if (st) return st;
        }
        for (uint32_t k = 0; k < nb; ++k) {
            const int s = grb::close_frame(c, fe, pre, k, status_out, [&] { return V.judge(c, k); });
            if (s == GR_OK) ++ic->n;
        }
    }
    return fe.finish(c);
}

}  // namespace

extern "C" {

gr_internals *gr_internals_create(gr_ctx *c, int kind, const uint64_t *atoms, uint64_t n_tuples, uint32_t flags, const float *axis, int *status) try {
    int dummy; if (!status) status = &dummy;
    if (!c) { *status = GR_E_INVALID_ARG; return nullptr; }
    *status = busy_check(c); if (*status) return nullptr;
    if (kind != GR_IC_DISTANCE && kind != GR_IC_ANGLE && kind != GR_IC_DIHEDRAL && kind != GR_IC_AXIS) { *status = fail(c, GR_E_INVALID_ARG, "internals: unknown kind"); return nullptr; }
    if (!atoms || n_tuples == 0 || n_tuples > 0x7FFFFFFFu) { *status = fail(c, GR_E_INVALID_ARG, "internals: the list of tuples is empty (or holds 2^31 tuples or more)"); return nullptr; }
    if ((flags & ~GR_IC_PBC) != 0u) { *status = fail(c, GR_E_INVALID_ARG, "internals: unknown flag"); return nullptr; }
    if (c->frame_stride * sizeof(float) >= GR_BUF_NOWHERE) { *status = fail(c, GR_E_INVALID_ARG, "internals: a slot of this system is too large for a buffer resource"); return nullptr; }
    std::unique_ptr<gr_internals> ic(new gr_internals());
    ic->c = c; ic->kind = kind; ic->flags = flags; ic->arity = (uint32_t)ic_arity(kind); ic->T = (uint32_t)n_tuples;
    ic->tpad = (ic->T + GR_IC_WG - 1u) & ~(GR_IC_WG - 1u);
    if (kind == GR_IC_AXIS) {
        if (!axis) { *status = fail(c, GR_E_INVALID_ARG, "internals: the axis kind needs an axis"); return nullptr; }
        const double x = axis[0], y = axis[1], z = axis[2], len = sqrt(x * x + y * y + z * z);
        if (!std::isfinite(len) || !(len > 0.0)) { *status = fail(c, GR_E_INVALID_ARG, "internals: the axis is zero or not finite"); return nullptr; }
        ic->axis[0] = (float)(x / len); ic->axis[1] = (float)(y / len); ic->axis[2] = (float)(z / len);
    }
    *status = ic->tab.build(c, "internals", "an atom appears twice in one tuple", atoms, n_tuples, ic->arity, ic->tpad); if (*status) return nullptr;
    bool ok = ic->verdicts.reserve(2u * GR_IC_AHEAD) && ic->o.reserve(ic->tpad, grbuf::exact) == hipSuccess && ic->s.reserve(ic->tpad, grbuf::exact) == hipSuccess &&
              ic->q.reserve(ic->tpad, grbuf::exact) == hipSuccess;
    ok = ok && ic_zero(ic.get()) == GR_OK && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        *status = fail(c, GR_E_HIP, "internals: device allocation failed");
        return nullptr;
    }
    *status = GR_OK;
    return ic.release();
} catch (...) { if (status) *status = gr_abi_guard(); return nullptr; }

void gr_internals_destroy(gr_internals *ic) try { gr_object_destroy(ic); } catch (...) { }

uint64_t gr_internals_count(const gr_internals *ic) { return ic ? ic->T : 0u; }
uint64_t gr_internals_frames(const gr_internals *ic) { return ic ? ic->n : 0u; }

int gr_internals_values_batch(gr_internals *ic, uint32_t first_slot, uint32_t n_frames, float *out, int *status_out) try {
    if (!ic) return GR_E_INVALID_ARG;
    int st = busy_check(ic->c); if (st) return st;
    if (!out) return fail(ic->c, GR_E_INVALID_ARG, "internals: no output array");
    return ic_values(ic, first_slot, n_frames, out, nullptr, ic->T, status_out);
} catch (...) { return gr_abi_guard(); }

int gr_internals_values_batch_device(gr_internals *ic, uint32_t first_slot, uint32_t n_frames, float *out_dev, uint64_t ld, int *status_out) try {
    if (!ic) return GR_E_INVALID_ARG;
    int st = busy_check(ic->c); if (st) return st;
    if (!out_dev || ld < ic->T) return fail(ic->c, GR_E_INVALID_ARG, "internals: no output array, or rows shorter than the number of tuples");
    return ic_values(ic, first_slot, n_frames, nullptr, out_dev, ld, status_out);
} catch (...) { return gr_abi_guard(); }

int gr_internals_accumulate_batch(gr_internals *ic, uint32_t first_slot, uint32_t n_frames, int *status_out) try {
    if (!ic) return GR_E_INVALID_ARG;
    int st = busy_check(ic->c); if (st) return st;
    return ic_accumulate(ic, first_slot, n_frames, status_out);
} catch (...) { return gr_abi_guard(); }

int gr_internals_clear(gr_internals *ic) try {
    if (!ic) return GR_E_INVALID_ARG;
    int st = busy_check(ic->c); if (st) return st;
    (void)hipSetDevice(ic->c->device);
    return ic_zero(ic);
} catch (...) { return gr_abi_guard(); }

int gr_internals_read_raw(gr_internals *ic, float *origin, double *sum, double *sumsq, uint64_t *n) try {
    if (!ic) return GR_E_INVALID_ARG;
    int st = busy_check(ic->c); if (st) return st;
    std::vector<float> o; std::vector<double> s, q;
    if (origin || sum || sumsq) { st = ic_get(ic, o, s, q); if (st) return st; }
    if (origin) memcpy(origin, o.data(), o.size() * sizeof(float));
    if (sum) memcpy(sum, s.data(), s.size() * sizeof(double));
    if (sumsq) memcpy(sumsq, q.data(), q.size() * sizeof(double));
    if (n) *n = ic->n;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_internals_read(gr_internals *ic, double *mean, double *var) try {
    if (!ic) return GR_E_INVALID_ARG;
    int st = busy_check(ic->c); if (st) return st;
    if (ic->n == 0) return fail(ic->c, GR_E_INVALID_ARG, "internals: no frame has been counted");
    std::vector<float> o; std::vector<double> s, q;
    st = ic_get(ic, o, s, q); if (st) return st;
    const double dn = (double)ic->n;
    for (size_t t = 0; t < ic->T; ++t) {
        double m = (double)o[t] + s[t] / dn;
        if (ic->kind == GR_IC_DIHEDRAL) m = ic_wrap_pi(m);
        if (mean) mean[t] = m;
        if (var) var[t] = std::max(q[t] - s[t] * s[t] / dn, 0.0) / dn;
    }
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_internals_merge(gr_internals *dst, gr_internals *src) try {
    if (!dst || !src) return GR_E_INVALID_ARG;
    gr_ctx *c = dst->c;
    int st = busy_check(c); if (st) return st;
    if (src->c != c) { st = busy_check(src->c); if (st) return fail(c, st, src->c->err); }
    if (src == dst) return fail(c, GR_E_INVALID_ARG, "internals: an object cannot be merged into itself");
    if (dst->kind != src->kind || dst->flags != src->flags || dst->T != src->T || dst->tab.tuples != src->tab.tuples || memcmp(dst->axis, src->axis, sizeof dst->axis) != 0) {
        c->counts[0] = dst->T; c->counts[1] = src->T;
        return fail(c, GR_E_INCONSISTENT_GROUP, "internals: the objects differ in kind, flags, axis or tuples");
    }
    if (src->n == 0) return GR_OK;
    std::vector<float> os, od; std::vector<double> ss, qs, sd, qd;
    st = ic_get(src, os, ss, qs); if (st) return src->c == c ? st : fail(c, st, src->c->err);
    if (dst->n == 0) {                                     // an empty object takes the other's origin and sums as they are
        st = ic_put(dst, os, ss, qs); if (st) return st;
        dst->n = src->n;
        return GR_OK;
    }
    st = ic_get(dst, od, sd, qd); if (st) return st;
    // src's sums moved to dst's origin: d' = d + delta with delta = o_src - o_dst (a dihedral's: the shorter way round)
    const double ns = (double)src->n;
    for (size_t t = 0; t < od.size(); ++t) {
        double delta = (double)os[t] - (double)od[t];
        if (dst->kind == GR_IC_DIHEDRAL) delta = ic_wrap_pi(delta);
        sd[t] += ss[t] + ns * delta;
        qd[t] += qs[t] + 2.0 * delta * ss[t] + ns * delta * delta;
    }
    st = ic_put(dst, od, sd, qd); if (st) return st;
    dst->n += src->n;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_internals_set_launch(gr_internals *ic, uint32_t tuple_ranges, uint32_t frame_chunk) try {
    if (!ic) return GR_E_INVALID_ARG;
    ic->tuple_ranges = tuple_ranges; ic->frame_chunk = frame_chunk;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_internals_stat(const gr_internals *ic, int key, uint64_t *value) try {
    if (!ic || !value) return GR_E_INVALID_ARG;
    switch (key) {
    case GR_IC_STAT_LAUNCHES: *value = ic->launches; return GR_OK;
    case GR_IC_STAT_LAST_RANGE_GROUPS: *value = ic->last_wx; return GR_OK;
    case GR_IC_STAT_LAST_FRAME_GROUPS: *value = ic->last_wy; return GR_OK;
    case GR_IC_STAT_LAST_CHECK_GROUPS: *value = ic->last_check; return GR_OK;
    case GR_IC_STAT_ARITY: *value = ic->arity; return GR_OK;
    case GR_IC_STAT_UNIQUE_ATOMS: *value = ic->tab.uniq.atoms.size(); return GR_OK;
    case GR_IC_STAT_AHEAD: *value = GR_IC_AHEAD; return GR_OK;
    default: return GR_E_INVALID_ARG;
    }
} catch (...) { return gr_abi_guard(); }

}  // extern "C"

#endif  // __HIPCC__
