// gr_series.h -- what the objects over batches of resident frames share on the host (RMSDPanel, Fluctuations, Covariance, MSD, Internals,
// VectorCorrelation): the atoms an object watches, the table of its tuples, the round of per-frame verdicts, and its end.
//   GrSnapshot    the atoms as a selection of the object's own (the group may be replaced or removed while the object lives): the
//                 ascending list on host and device, the FORM in which k_fl_check walks it -- 0: a contiguous block, 1: index list,
//                 2: masked span (at least half of the span's atoms are the group's; one bit per atom of the system) --, its UNITS
//                 (4-atom groups of the span, or list entries) and the GrSel
//   GrTuples      T tuples of 2 .. 4 atoms: the caller's list, the unique atoms as an index-list snapshot, and the device table
//                 uint32 [arity][pad], component-major, so that a wave's index loads are contiguous
//   GrVerdicts    one word per frame of a segment: GR_NOIDX (every atom has a position), GR_FL_SKIP (the frame failed its host checks,
//                 no kernel touches it) or the lowest atom without position.  begin() fills and uploads them, check() launches
//                 k_fl_check, the object's own kernels read them, end() brings them back and judge() closes a frame with them.
//                 `tail` words behind the segment's last say "skip": the walks request the verdicts of a turn of their ring one turn ahead.
//   k_fl_check    read-only pass over the x rows: the first atom of the snapshot without position, per frame (atomicMin into the
//                 frame's verdict word).  A frame with such an atom is counted for NO atom.
#pragma once
#include "gr_kernels.h"

#if defined(__HIPCC__)

#define GR_FL_SKIP 0xFFFFFFFEu            /* verdict word: the frame failed its host checks, no kernel touches it (GR_NOIDX: every atom has a position) */
#define GR_FL_CHECK_WGS 4096u             /* k_fl_check's grid along x at most */

namespace {

__global__ __launch_bounds__(256) void k_fl_check(const float *__restrict__ frames, size_t stride, uint32_t s0, GrSel sel, int form, uint32_t *verdict) {
    const uint32_t f = blockIdx.y;
    if (verdict[f] == GR_FL_SKIP) return;
    const float *xyz = frames + (size_t)(s0 + f) * stride;
    const uint32_t step = gridDim.x * 256u;
    uint32_t bad = GR_NOIDX;
    if (form == 1) {
        for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < sel.n; k += step) {
            const uint32_t i = sel.idx[k];
            const float x = xyz[gr_tile_index(i, 0)];
            if (x != x) bad = min(bad, i);
        }
    } else {
        const float4 *f4 = reinterpret_cast<const float4 *>(xyz);
        const uint32_t a0 = sel.start, a1 = sel.start + sel.span;
        for (uint32_t g = (a0 >> 2) + blockIdx.x * 256u + threadIdx.x; g <= (a1 - 1u) >> 2; g += step) {
            const size_t b = gr_row_index(g, 0);
            const float4 r0 = f4[b], r1 = f4[b + 64];     // x of the lane's atoms: row 0 .x .y, row 1 .z .w
            const float x[4] = { r0.x, r0.y, r1.z, r1.w };
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t i = 4u * g + (uint32_t)k;
                const bool in = i >= a0 && i < a1 && (form == 0 || ((sel.mask[i >> 5] >> (i & 31u)) & 1u));
                if (in && x[k] != x[k]) bad = min(bad, i);
            }
        }
    }
    // (rare: a wave that has such an atom reduces and reports it, the others do nothing)
    if (__builtin_amdgcn_ballot_w64(bad != GR_NOIDX) != 0ull) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) bad = min(bad, (uint32_t)__shfl_xor((int)bad, off, 64));
        if ((threadIdx.x & 63u) == 0u) atomicMin(&verdict[f], bad);
    }
}

struct GrSnapshot {
    std::vector<uint32_t> atoms;          // ascending, each once
    grbuf::Dev<uint32_t> atoms_dev, mask_dev;
    int form = 0;
    uint32_t units = 0;
    GrSel sel = {};

    // from a sorted list that is not empty (the caller has set the device); as_list: form 1 whatever the shape, so that sums over the
    // snapshot are added in the order of its ordinals.  false: a device allocation or copy failed
    bool build(const gr_ctx *c, std::vector<uint32_t> sorted, bool as_list = false) {
        atoms = std::move(sorted);
        const uint32_t n = (uint32_t)atoms.size(), a0 = atoms.front(), span = atoms.back() - a0 + 1u;
        form = as_list ? 1 : (span == n ? 0 : (2ull * n >= span ? 2 : 1));
        units = form == 1 ? n : ((a0 + span - 1u) >> 2) - (a0 >> 2) + 1u;
        bool ok = atoms_dev.reserve(n, grbuf::exact) == hipSuccess && hipMemcpy(atoms_dev.get(), atoms.data(), 4 * (size_t)n, hipMemcpyHostToDevice) == hipSuccess;
        if (ok && form == 2) {
            std::vector<uint32_t> bits(((size_t)c->n_pad + 31) / 32, 0u);
            for (uint32_t a : atoms) bits[a >> 5] |= 1u << (a & 31u);
            ok = mask_dev.reserve(bits.size(), grbuf::exact) == hipSuccess && hipMemcpy(mask_dev.get(), bits.data(), 4 * bits.size(), hipMemcpyHostToDevice) == hipSuccess;
        }
        sel.n = n; sel.contiguous = form == 0 ? 1u : 0u; sel.start = a0; sel.g0 = a0 >> 8; sel.idx = atoms_dev.get();
        sel.masked = form == 2 ? 1u : 0u; sel.span = span; sel.mask = form == 2 ? mask_dev.get() : nullptr;
        return ok;
    }
};

struct GrTuples {
    std::vector<uint32_t> tuples;         // [T][arity], the caller's order
    GrSnapshot uniq;                      // the atoms the tuples name, as an index list for k_fl_check
    grbuf::Dev<uint32_t> table_dev;       // [arity][pad]

    // n tuples of `arity` atoms, pad >= n entries per component.  GR_E_OUT_OF_RANGE with the atom, GR_E_INVALID_ARG with the tuple that
    // names an atom twice (`twice` is the object's sentence for it), GR_E_HIP; `who` opens the messages
    int build(gr_ctx *c, const char *who, const char *twice, const uint64_t *atoms, uint64_t n, uint32_t arity, uint32_t pad) {
        const uint32_t A = arity;
        tuples.resize((size_t)n * A);
        for (uint64_t t = 0; t < n; ++t) {
            for (uint32_t a = 0; a < A; ++a) {
                const uint64_t i = atoms[t * A + a];
                if (i >= c->n) return fail(c, GR_E_OUT_OF_RANGE, std::string(who) + ": atom index out of range", i);
                for (uint32_t b = 0; b < a; ++b)
                    if (atoms[t * A + b] == i) return fail(c, GR_E_INVALID_ARG, std::string(who) + ": " + twice, t);
                tuples[t * A + a] = (uint32_t)i;
            }
        }
        std::vector<uint32_t> u = tuples;
        std::sort(u.begin(), u.end());
        u.erase(std::unique(u.begin(), u.end()), u.end());
        std::vector<uint32_t> table((size_t)A * pad, 0u);
        for (uint64_t t = 0; t < n; ++t)
            for (uint32_t a = 0; a < A; ++a) table[(size_t)a * pad + t] = tuples[(size_t)t * A + a];
        (void)hipSetDevice(c->device);
        if (!uniq.build(c, std::move(u), true) || table_dev.reserve(table.size(), grbuf::exact) != hipSuccess ||
            hipMemcpy(table_dev.get(), table.data(), 4 * table.size(), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, GR_E_HIP, std::string(who) + ": device allocation failed");
        }
        return GR_OK;
    }
};

struct GrVerdicts {
    grbuf::Dev<uint32_t> dev;
    grbuf::Pinned<uint32_t> host;
    uint32_t tail = 0;

    bool reserve(uint32_t tail_words) {
        tail = tail_words;
        return dev.reserve(GR_MAX_BATCH + tail, grbuf::exact) == hipSuccess && host.reserve(GR_MAX_BATCH + tail, grbuf::exact) == hipSuccess;
    }
    // clean where the host checks passed, "skip" elsewhere and in the tail
    int begin(gr_ctx *c, const grb::Prechecks &pre, uint32_t nb) {
        uint32_t *vh = host.get();
        for (uint32_t k = 0; k < nb; ++k) vh[k] = pre.ok(k) ? GR_NOIDX : GR_FL_SKIP;
        for (uint32_t k = nb; k < nb + tail; ++k) vh[k] = GR_FL_SKIP;
        HIPCHK(c, hipMemcpyAsync(dev.get(), vh, (nb + tail) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        return GR_OK;
    }
    // 256 units per workgroup of the check, up to GR_FL_CHECK_WGS that stride; cap (an object's set_launch) lowers the grid.  Returns the grid.
    uint32_t check(gr_ctx *c, const GrSnapshot &s, uint32_t s0, uint32_t nb, uint32_t cap = 0) {
        uint32_t grid = std::min<uint32_t>((s.units + 255u) / 256u, GR_FL_CHECK_WGS);
        if (cap && cap < grid) grid = cap;
        k_fl_check<<<dim3(grid, nb), dim3(256), 0, c->stream>>>(c->frames, c->frame_stride, s0, s.sel, s.form, dev.get());
        return grid;
    }
    int end(gr_ctx *c, uint32_t nb) {
        HIPCHK(c, hipMemcpyAsync(host.get(), dev.get(), nb * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return GR_OK;
    }
    // frame k of the segment, behind end()
    int judge(gr_ctx *c, uint32_t k) const {
        const uint32_t v = host.get()[k];
        return v != GR_NOIDX ? fail(c, GR_E_NO_POSITION, "atom has no position", v) : (int)GR_OK;
    }
};

// the end of an object that owns grow-only buffers on its context's device (inside the entry point's try)
template <class Obj>
void gr_object_destroy(Obj *o) {
    if (!o) return;
    (void)hipSetDevice(o->c->device);
    (void)hipStreamSynchronize(o->c->stream);
    delete o;                                              // (frees the grow-only buffers)
}

}  // namespace

#endif  // __HIPCC__
