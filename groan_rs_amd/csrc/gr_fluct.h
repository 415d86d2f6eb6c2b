// gr_fluct.h -- Fluctuations: the mean structure and the per-atom RMSF of a group over batches of resident frames.
//
// The reference has no such function: its users write the loop around calc_rmsd_and_fit themselves (download every fitted frame, add it
// up).  Here the loop is the library's.  Per atom and component the object keeps, on the device,
//   o  (f32)  the ORIGIN: the atom's position in the first frame the object ever counted
//   s  (f64)  sum of d            d = x - o, ONE f32 subtraction, then widened
//   q  (f64)  sum of d * d        (the product of two widened f32 is exact in f64: the fused multiply-add rounds once, like mul + add)
// and the host closes them in f64: mean = o + s / n, var_c = max(q_c - s_c^2 / n, 0) / n, rmsf = sqrt(var_x + var_y + var_z).
// ORDER OF THE SUMS: a lane owns its atoms for the whole launch and adds the frames in ascending order, one after another; nothing is
// split over frames, no atomic touches a sum.  So s and q are a function of the SEQUENCE of counted frames alone -- not of how the frames
// were cut into calls, 1024-frame segments or grids -- and tests/fluct_ref.py restates them bit for bit in three lines of numpy.
//   k_fl_check        (gr_series.h, with the snapshot and the round of verdicts) the first atom of the group without position, per frame.
//                     A frame with such an atom is counted for NO atom.
//   k_fl_accumulate   one wave per range of the group's UNITS (4-atom groups of the span for a contiguous or masked group, list entries
//                     for an index list).  A lane loads the state of its unit, walks the segment's frames with the rows of GR_FL_AHEAD
//                     frames in flight (buffer loads: a frame beyond the segment is a resource of zero records, a unit beyond the range an
//                     offset beyond every slot -- no load carries a condition), skips the frames whose verdict is not clean (a branch
//                     that is the same in every lane) and writes the state back.
//                     <false>: the state of a unit is kept in the ROW ORDER of gr_layout.h (x0 x1 y0 y1 | z0 z1 x2 x3 | y2 y3 z2 z3), so
//                              d is row minus origin, component by component, and nothing is unpacked; components of pads and of atoms
//                              outside the group get d = 0 whatever the frame holds there
//                     <true>:  one atom per lane, three dword loads per frame
//   k_fl_store_mean   the mean, rounded to f32, into the group's atoms of one slot (gr_pos_store)
// STATE LAYOUT: component-major in pieces of 16 bytes per unit -- float4 [3][units] for o, double2 [6][units] for s and for q (index list:
// float [3][units], double [3][units]) -- so every state load and store of a wave is one contiguous block.
#pragma once
#include "gr_series.h"

#if defined(__HIPCC__)

#define GR_FL_AHEAD 8                     /* frames whose rows a lane has in flight */
#define GR_FL_WG 64u                      /* lanes of a workgroup of k_fl_accumulate: one wave */
#define GR_FL_MAX_RANGES (1u << 22)       /* k_fl_accumulate's grid at most */

struct GrFlState {
    float *o;                             // [C][upad], C = 12 (rows) or 3 (index list) components per unit
    double *s, *q;
    uint32_t upad;                        // units, rounded up to the wave
};

struct gr_fluct {
    gr_ctx *c = nullptr;
    std::string group;
    GrSnapshot snap;                      // the group's atoms at create
    GrVerdicts verdicts;
    uint32_t n_atoms = 0, upad = 0;       // ..., the snapshot's units rounded up to the wave
    grbuf::Dev<float> o, mean_dev;        // [C * upad], [n_atoms][3]
    grbuf::Dev<double> s, q;              // [C * upad]
    uint64_t n = 0;                       // counted frames
    uint32_t range_groups = 0, check_groups = 0;      // gr_fluct_set_launch; 0: the default
    uint32_t last_wx = 0, last_check = 0;             // grids of the last segment that was launched
    uint64_t launches = 0;
};

typedef double gr_fl_d2 __attribute__((ext_vector_type(2)));

namespace {

__device__ __forceinline__ float fl_buf_load_f32_stream(__amdgpu_buffer_rsrc_t r, uint32_t byte_off) {
    return __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)byte_off, 0, 2 /* nt */));
}

// frames [s0, s0 + nf) of `frames`, verdict[f] per frame and GR_FL_SKIP in verdict[nf .. nf + 2 * GR_FL_AHEAD); have_origin: the object has counted a frame before this launch
template <bool LIST>
__global__ __launch_bounds__(GR_FL_WG) void k_fl_accumulate(const float *__restrict__ frames, size_t stride, uint32_t slot_bytes, uint32_t s0, uint32_t nf, GrSel sel,
                                                            int form, const uint32_t *__restrict__ verdict, GrFlState S, uint32_t have_origin) {
    constexpr int C = LIST ? 3 : 12;
    // the workgroup's range of units: 4-atom groups of the span (contiguous, masked) or list entries
    const uint32_t a0 = sel.start, a1 = sel.start + sel.span;
    const uint32_t ubase = LIST ? 0u : a0 >> 2;
    const uint32_t units = LIST ? sel.n : ((a1 - 1u) >> 2) - (a0 >> 2) + 1u;
    const uint32_t per = (units + gridDim.x - 1u) / gridDim.x;
    const uint32_t u0 = (uint32_t)min((uint64_t)blockIdx.x * per, (uint64_t)units), u1 = (uint32_t)min((uint64_t)u0 + per, (uint64_t)units);
    const size_t up = S.upad;
    // the frame's slot as a buffer: zero records beyond the segment (and then the last frame's address, so that nothing points outside the slots)
    auto slot_of = [&](uint32_t f) {
        return gr_buf_rsrc(frames + (size_t)(s0 + min(f, nf - 1u)) * stride, f < nf ? slot_bytes : 0u);
    };
    for (uint32_t ub = u0; ub < u1; ub += GR_FL_WG) {
        const uint32_t u = ub + threadIdx.x;
        const bool live = u < u1;
        // where the lane's unit lies inside a slot, and which of its components belong to the group
        uint32_t off[3] = { GR_BUF_NOWHERE, GR_BUF_NOWHERE, GR_BUF_NOWHERE };
        bool in[C];
#pragma unroll
        for (int j = 0; j < C; ++j) in[j] = false;
        if (live) {
            if (LIST) {
                const uint32_t i = sel.idx[u];
#pragma unroll
                for (int c = 0; c < 3; ++c) { off[c] = (uint32_t)gr_tile_index(i, c) * 4u; in[c] = true; }
            } else {
                const uint32_t g = ubase + u;
                off[0] = (uint32_t)gr_row_index(g, 0) * 16u;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t i = 4u * g + (uint32_t)k;
                    const bool a = i >= a0 && i < a1 && (form == 0 || ((sel.mask[i >> 5] >> (i & 31u)) & 1u));
#pragma unroll
                    for (int c = 0; c < 3; ++c) in[(k >> 1) * 6 + 2 * c + (k & 1)] = a;      // (the row order: gr_tile_index's `s`)
                }
            }
        }
        auto request = [&](uint32_t f, float (&v)[C]) {
            const __amdgpu_buffer_rsrc_t rs = slot_of(f);
            if (LIST) {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = fl_buf_load_f32_stream(rs, off[c]);
            } else {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float4 t = gr_buf_load_stream(rs, off[0] + 1024u * (uint32_t)r);
                    v[4 * r] = t.x; v[4 * r + 1] = t.y; v[4 * r + 2] = t.z; v[4 * r + 3] = t.w;
                }
            }
        };
        // the unit's state (requested BEFORE the first rows: loads return in order, and a state load behind the rows would make the
        // first sum of every trip through the loop wait for every row in flight)
        float o[C];
        double s[C], q[C];
#pragma unroll
        for (int j = 0; j < C; ++j) { o[j] = 0.0f; s[j] = 0.0; q[j] = 0.0; }
        if (live) {
            if (LIST) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { o[c] = S.o[c * up + u]; s[c] = S.s[c * up + u]; q[c] = S.q[c * up + u]; }
            } else {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float4 t = reinterpret_cast<const float4 *>(S.o)[r * up + u];
                    o[4 * r] = t.x; o[4 * r + 1] = t.y; o[4 * r + 2] = t.z; o[4 * r + 3] = t.w;
                }
#pragma unroll
                for (int p = 0; p < 6; ++p) {
                    const gr_fl_d2 ts = reinterpret_cast<const gr_fl_d2 *>(S.s)[p * up + u], tq = reinterpret_cast<const gr_fl_d2 *>(S.q)[p * up + u];
                    s[2 * p] = ts.x; s[2 * p + 1] = ts.y; q[2 * p] = tq.x; q[2 * p + 1] = tq.y;
                }
            }
        }
        float ring[GR_FL_AHEAD][C];
#pragma unroll
        for (int k = 0; k < GR_FL_AHEAD; ++k) {
            request((uint32_t)k, ring[k]);
            __builtin_amdgcn_sched_barrier(0);      // in frame order: left to itself the scheduler requests frame 0 last, and the first sum of every turn of the ring waits for all rows
        }
        bool have = have_origin != 0u;
        // the verdicts of a turn of the ring are requested one turn ahead (2 * GR_FL_AHEAD words behind the segment's last say "skip"):
        // read frame by frame, every frame would wait for a scalar load of its own
        uint32_t vnext[GR_FL_AHEAD];
#pragma unroll
        for (int k = 0; k < GR_FL_AHEAD; ++k) vnext[k] = verdict[k];
        for (uint32_t base = 0; base < nf; base += GR_FL_AHEAD) {
            uint32_t vcur[GR_FL_AHEAD];
#pragma unroll
            for (int k = 0; k < GR_FL_AHEAD; ++k) { vcur[k] = vnext[k]; vnext[k] = verdict[base + GR_FL_AHEAD + (uint32_t)k]; }
#pragma unroll
            for (int k = 0; k < GR_FL_AHEAD; ++k) {
                const uint32_t f = base + (uint32_t)k;
                const float (&v)[C] = ring[k];
                if (f < nf && vcur[k] == GR_NOIDX) {
                    if (!have) {
#pragma unroll
                        for (int j = 0; j < C; ++j) o[j] = in[j] ? v[j] : 0.0f;
                        have = true;
                    }
#pragma unroll
                    for (int j = 0; j < C; ++j) {
                        const float d = in[j] ? v[j] - o[j] : 0.0f;
                        const double dd = (double)d;
                        s[j] += dd;
                        q[j] = fma(dd, dd, q[j]);
                    }
                }
                // (behind the sums: the rows then land in the registers the frame has just left, and the turn of the ring moves nothing)
                request(f + GR_FL_AHEAD, ring[k]);
            }
        }
        if (live) {
            if (LIST) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { S.o[c * up + u] = o[c]; S.s[c * up + u] = s[c]; S.q[c * up + u] = q[c]; }
            } else {
#pragma unroll
                for (int r = 0; r < 3; ++r) reinterpret_cast<float4 *>(S.o)[r * up + u] = make_float4(o[4 * r], o[4 * r + 1], o[4 * r + 2], o[4 * r + 3]);
#pragma unroll
                for (int p = 0; p < 6; ++p) {
                    gr_fl_d2 ts, tq;
                    ts.x = s[2 * p]; ts.y = s[2 * p + 1]; tq.x = q[2 * p]; tq.y = q[2 * p + 1];
                    reinterpret_cast<gr_fl_d2 *>(S.s)[p * up + u] = ts; reinterpret_cast<gr_fl_d2 *>(S.q)[p * up + u] = tq;
                }
            }
        }
    }
}

// mean[k][3] -> atom atoms[k] of the slot; an atom whose mean is not a number in one component has no position (NaN in all three)
__global__ __launch_bounds__(256) void k_fl_store_mean(float *__restrict__ xyz, const uint32_t *__restrict__ atoms, const float *__restrict__ mean, uint32_t n) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    float x = mean[3u * k], y = mean[3u * k + 1u], z = mean[3u * k + 2u];
    if (x != x || y != y || z != z) x = y = z = __uint_as_float(0x7fc00000u);
    gr_pos_store(xyz, atoms[k], x, y, z);
}

// element of component c of the group's k-th atom inside a state array whose pieces hold V values (4: o, 2: s and q; the index list: 1)
size_t fl_at(const gr_fluct *f, uint32_t k, int c, uint32_t V) {
    if (f->snap.form == 1) return (size_t)c * f->upad + k;
    const uint32_t i = f->snap.atoms[k], u = (i >> 2) - (f->snap.atoms[0] >> 2), j = ((i >> 1) & 1u) * 6u + 2u * (uint32_t)c + (i & 1u);
    return (size_t)(j / V) * f->upad * V + (size_t)u * V + j % V;
}
size_t fl_state_len(const gr_fluct *f) { return (size_t)(f->snap.form == 1 ? 3u : 12u) * f->upad; }

// the state in group order, [n_atoms][3] each
int fl_get(gr_fluct *f, std::vector<float> &o, std::vector<double> &s, std::vector<double> &q) {
    gr_ctx *c = f->c;
    (void)hipSetDevice(c->device);
    const size_t len = fl_state_len(f);
    std::vector<float> od(len); std::vector<double> sd(len), qd(len);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(od.data(), f->o.get(), len * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(sd.data(), f->s.get(), len * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(qd.data(), f->q.get(), len * sizeof(double), hipMemcpyDeviceToHost));
    const size_t S = f->n_atoms;
    o.resize(3 * S); s.resize(3 * S); q.resize(3 * S);
    const uint32_t vo = f->snap.form == 1 ? 1u : 4u, vs = f->snap.form == 1 ? 1u : 2u;
    for (uint32_t k = 0; k < f->n_atoms; ++k)
        for (int a = 0; a < 3; ++a) { o[3 * (size_t)k + a] = od[fl_at(f, k, a, vo)]; s[3 * (size_t)k + a] = sd[fl_at(f, k, a, vs)]; q[3 * (size_t)k + a] = qd[fl_at(f, k, a, vs)]; }
    return GR_OK;
}

// ... and back (components of pads and of atoms outside the group are zero, as the kernel keeps them)
int fl_put(gr_fluct *f, const std::vector<float> &o, const std::vector<double> &s, const std::vector<double> &q) {
    gr_ctx *c = f->c;
    (void)hipSetDevice(c->device);
    const size_t len = fl_state_len(f);
    std::vector<float> od(len, 0.0f); std::vector<double> sd(len, 0.0), qd(len, 0.0);
    const uint32_t vo = f->snap.form == 1 ? 1u : 4u, vs = f->snap.form == 1 ? 1u : 2u;
    for (uint32_t k = 0; k < f->n_atoms; ++k)
        for (int a = 0; a < 3; ++a) { od[fl_at(f, k, a, vo)] = o[3 * (size_t)k + a]; sd[fl_at(f, k, a, vs)] = s[3 * (size_t)k + a]; qd[fl_at(f, k, a, vs)] = q[3 * (size_t)k + a]; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(f->o.get(), od.data(), len * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(f->s.get(), sd.data(), len * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(f->q.get(), qd.data(), len * sizeof(double), hipMemcpyHostToDevice));
    return GR_OK;
}

int fl_zero(gr_fluct *f) {
    gr_ctx *c = f->c;
    const size_t len = fl_state_len(f);
    HIPCHK(c, hipMemsetAsync(f->o.get(), 0, len * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(f->s.get(), 0, len * sizeof(double), c->stream));
    HIPCHK(c, hipMemsetAsync(f->q.get(), 0, len * sizeof(double), c->stream));
    f->n = 0;
    return GR_OK;
}

// the closing formulas, one component: mean and variance of n counted frames
void fl_close(float o, double s, double q, uint64_t n, double &mean, double &var) {
    if (n == 0) { mean = NAN; var = NAN; return; }
    const double dn = (double)n;
    mean = (double)o + s / dn;
    var = std::max(q - s * s / dn, 0.0) / dn;
}

int fl_accumulate(gr_fluct *f, uint32_t first_slot, uint32_t n_frames, int *status_out) {
    gr_ctx *c = f->c;
    int st = slot_check(c, first_slot, n_frames); if (st) return st;
    (void)hipSetDevice(c->device);
    const GrSel sel = f->snap.sel;
    const int form = f->snap.form;
    const uint32_t slot_bytes = (uint32_t)(c->frame_stride * sizeof(float));
    const GrFlState S = { f->o.get(), f->s.get(), f->q.get(), f->upad };
    GrVerdicts &V = f->verdicts;
    const uint32_t *vd = V.dev.get();
    grb::FirstError<gr_ctx> fe;
    for (const auto [b0, nb, s0] : grb::Segments{ first_slot, n_frames }) {
        const grb::Prechecks pre(c, { b0, nb, s0 }, box_checks(c, false));
        if (pre.any_ok) {
            SlotUse use(c, s0, nb);
            st = V.begin(c, pre, nb); if (st) return st;
            // launch geometry: one wave per 64 units; gr_fluct_set_launch replaces the number of ranges and caps the check's grid
            const uint32_t wx = std::min<uint32_t>(f->range_groups ? f->range_groups : (f->snap.units + GR_FL_WG - 1u) / GR_FL_WG, GR_FL_MAX_RANGES);
            const uint32_t check = V.check(c, f->snap, s0, nb, f->check_groups);
            if (form == 1) k_fl_accumulate<true><<<dim3(wx), dim3(GR_FL_WG), 0, c->stream>>>(c->frames, c->frame_stride, slot_bytes, s0, nb, sel, form, vd, S, f->n ? 1u : 0u);
            else k_fl_accumulate<false><<<dim3(wx), dim3(GR_FL_WG), 0, c->stream>>>(c->frames, c->frame_stride, slot_bytes, s0, nb, sel, form, vd, S, f->n ? 1u : 0u);
            HIPCHK(c, hipGetLastError());
            ++f->launches; f->last_wx = wx; f->last_check = check;
            st = V.end(c, nb); if (st) return st;
        }
        for (uint32_t k = 0; k < nb; ++k) {
            const int s = grb::close_frame(c, fe, pre, k, status_out, [&] { return V.judge(c, k); });
            if (s == GR_OK) ++f->n;
        }
    }
    return fe.finish(c);
}

}  // namespace

extern "C" {

gr_fluct *gr_fluct_create(gr_ctx *c, const char *group, int *status) try {
    int dummy; if (!status) status = &dummy;
    if (!c) { *status = GR_E_INVALID_ARG; return nullptr; }
    *status = busy_check(c); if (*status) return nullptr;
    const Group *g = need_group(c, group, *status, true); if (!g) return nullptr;
    if (c->frame_stride * sizeof(float) >= GR_BUF_NOWHERE) { *status = fail(c, GR_E_INVALID_ARG, "fluctuations: a slot of this system is too large for a buffer resource"); return nullptr; }
    std::unique_ptr<gr_fluct> f(new gr_fluct());
    f->c = c; f->group = group;
    (void)hipSetDevice(c->device);
    bool ok = f->snap.build(c, hb_group_atoms(*g)) && f->verdicts.reserve(2u * GR_FL_AHEAD);
    f->n_atoms = (uint32_t)f->snap.atoms.size();
    f->upad = (f->snap.units + GR_FL_WG - 1u) & ~(GR_FL_WG - 1u);
    const size_t len = fl_state_len(f.get());
    ok = ok && f->o.reserve(len, grbuf::exact) == hipSuccess && f->s.reserve(len, grbuf::exact) == hipSuccess && f->q.reserve(len, grbuf::exact) == hipSuccess &&
         f->mean_dev.reserve(3 * (size_t)f->n_atoms, grbuf::exact) == hipSuccess;
    ok = ok && fl_zero(f.get()) == GR_OK && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        *status = fail(c, GR_E_HIP, "fluctuations: device allocation failed");
        return nullptr;
    }
    *status = GR_OK;
    return f.release();
} catch (...) { if (status) *status = gr_abi_guard(); return nullptr; }

void gr_fluct_destroy(gr_fluct *f) try { gr_object_destroy(f); } catch (...) { }

int gr_fluct_accumulate_batch(gr_fluct *f, uint32_t first_slot, uint32_t n_frames, int *status_out) try {
    if (!f) return GR_E_INVALID_ARG;
    return fl_accumulate(f, first_slot, n_frames, status_out);
} catch (...) { return gr_abi_guard(); }

int gr_fluct_clear(gr_fluct *f) try {
    if (!f) return GR_E_INVALID_ARG;
    int st = busy_check(f->c); if (st) return st;
    (void)hipSetDevice(f->c->device);
    return fl_zero(f);
} catch (...) { return gr_abi_guard(); }

uint64_t gr_fluct_frames(const gr_fluct *f) { return f ? f->n : 0u; }
uint64_t gr_fluct_n_atoms(const gr_fluct *f) { return f ? f->n_atoms : 0u; }

int gr_fluct_read_raw(gr_fluct *f, float *origin, double *sum, double *sumsq, uint64_t *n) try {
    if (!f) return GR_E_INVALID_ARG;
    int st = busy_check(f->c); if (st) return st;
    std::vector<float> o; std::vector<double> s, q;
    if (origin || sum || sumsq) { st = fl_get(f, o, s, q); if (st) return st; }
    if (origin) memcpy(origin, o.data(), o.size() * sizeof(float));
    if (sum) memcpy(sum, s.data(), s.size() * sizeof(double));
    if (sumsq) memcpy(sumsq, q.data(), q.size() * sizeof(double));
    if (n) *n = f->n;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_fluct_read(gr_fluct *f, double *mean, double *var, double *rmsf) try {
    if (!f) return GR_E_INVALID_ARG;
    int st = busy_check(f->c); if (st) return st;
    std::vector<float> o; std::vector<double> s, q;
    st = fl_get(f, o, s, q); if (st) return st;
    for (size_t k = 0; k < f->n_atoms; ++k) {
        double sum = 0.0;
        for (int a = 0; a < 3; ++a) {
            double m, v;
            fl_close(o[3 * k + a], s[3 * k + a], q[3 * k + a], f->n, m, v);
            if (mean) mean[3 * k + a] = m;
            if (var) var[3 * k + a] = v;
            sum += v;
        }
        if (rmsf) rmsf[k] = sqrt(sum);
    }
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_fluct_merge(gr_fluct *dst, gr_fluct *src) try {
    if (!dst || !src) return GR_E_INVALID_ARG;
    gr_ctx *c = dst->c;
    int st = busy_check(c); if (st) return st;
    if (src->c != c) { st = busy_check(src->c); if (st) return fail(c, st, src->c->err); }
    if (dst->n_atoms != src->n_atoms) { c->counts[0] = dst->n_atoms; c->counts[1] = src->n_atoms; return fail(c, GR_E_INCONSISTENT_GROUP, dst->group); }
    if (src == dst) return fail(c, GR_E_INVALID_ARG, "fluctuations: an object cannot be merged into itself");
    if (src->n == 0) return GR_OK;
    std::vector<float> os, od; std::vector<double> ss, qs, sd, qd;
    st = fl_get(src, os, ss, qs); if (st) return src->c == c ? st : fail(c, st, src->c->err);
    if (dst->n == 0) {                                     // an empty object takes the other's origin and sums as they are
        st = fl_put(dst, os, ss, qs); if (st) return st;
        dst->n = src->n;
        return GR_OK;
    }
    st = fl_get(dst, od, sd, qd); if (st) return st;
    // src's sums moved to dst's origin: d' = d + delta with delta = o_src - o_dst
    const double ns = (double)src->n;
    for (size_t k = 0; k < od.size(); ++k) {
        const double delta = (double)os[k] - (double)od[k];
        sd[k] += ss[k] + ns * delta;
        qd[k] += qs[k] + 2.0 * delta * ss[k] + ns * delta * delta;
    }
    st = fl_put(dst, od, sd, qd); if (st) return st;
    dst->n += src->n;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_fluct_store_mean(gr_fluct *f, gr_ctx *dst, uint32_t slot) try {
    if (!f || !dst) return GR_E_INVALID_ARG;
    gr_ctx *c = f->c;
    int st = busy_check(c); if (st) return st;
    if (dst->device != c->device || dst->n != c->n) return fail(c, GR_E_INVALID_ARG, "fluctuations: the mean goes into a context on the same device with the same number of atoms");
    if (f->n == 0) return fail(c, GR_E_INVALID_ARG, "fluctuations: no frame has been counted, there is no mean");
    st = slot_check(dst, slot); if (st) return dst == c ? st : fail(c, st, dst->err);
    std::vector<float> o; std::vector<double> s, q;
    st = fl_get(f, o, s, q); if (st) return st;
    std::vector<float> mean(o.size());
    for (size_t k = 0; k < o.size(); ++k) { double m, v; fl_close(o[k], s[k], q[k], f->n, m, v); mean[k] = (float)m; }
    HIPCHK(c, hipMemcpy(f->mean_dev.get(), mean.data(), mean.size() * sizeof(float), hipMemcpyHostToDevice));
    {
        SlotUse use(dst, slot);
        k_fl_store_mean<<<dim3((f->n_atoms + 255u) / 256u), dim3(256), 0, dst->stream>>>(dst->frames + (size_t)slot * dst->frame_stride, f->snap.atoms_dev.get(), f->mean_dev.get(), f->n_atoms);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipStreamSynchronize(dst->stream));         // (the next call may rewrite mean_dev)
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_fluct_set_launch(gr_fluct *f, uint32_t range_groups, uint32_t check_groups) try {
    if (!f) return GR_E_INVALID_ARG;
    f->range_groups = range_groups; f->check_groups = check_groups;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_fluct_stat(const gr_fluct *f, int key, uint64_t *value) try {
    if (!f || !value) return GR_E_INVALID_ARG;
    switch (key) {
    case GR_FL_STAT_LAUNCHES: *value = f->launches; return GR_OK;
    case GR_FL_STAT_LAST_RANGE_GROUPS: *value = f->last_wx; return GR_OK;
    case GR_FL_STAT_LAST_CHECK_GROUPS: *value = f->last_check; return GR_OK;
    case GR_FL_STAT_FORM: *value = (uint64_t)f->snap.form; return GR_OK;
    case GR_FL_STAT_AHEAD: *value = GR_FL_AHEAD; return GR_OK;
    default: return GR_E_INVALID_ARG;
    }
} catch (...) { return gr_abi_guard(); }

}  // extern "C"

#endif  // __HIPCC__
