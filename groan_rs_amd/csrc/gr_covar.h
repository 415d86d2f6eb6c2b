// gr_covar.h -- Covariance: the positional covariance matrix (3S x 3S) and the dynamical cross-correlation map (S x S) of a group over
// batches of resident frames -- the step after Fluctuations in every essential-dynamics workflow (gmx covar); the reference has no function for it.
//
// Per snapshot of S atoms (group order, D = 3S, dimension 3k + c) the object keeps on the device
//   o  (f32) [D]      the ORIGIN: the atom's position in the first frame the object ever counted (Fluctuations' rule)
//   Q  (f64) [R][R]   sum over the counted frames of e e^T, e = (d_0 .. d_{D-1}, 1), d = x - o as ONE f32 subtraction, then widened; R = D + 1.
//                     Row / column D of Q is s = sum d, Q[D][D] the number of counted frames: s and n come out of the same product.
// and the host closes them in f64 (cv_close).  Only the upper BLOCK triangle of Q is stored, in blocks of GR_CV_BLOCK x GR_CV_BLOCK.
//   k_fl_check     (gr_series.h) the first atom of the group without position, per frame
//   k_cv_origin    the first clean frame of an empty object sets o
//   k_cv_pack      a segment of up to 1024 frames -> the dimension-major panel P[R_pad][K_pad] (f32, frames contiguous, K_pad a multiple of
//                  GR_CV_TRIP): P[r][f] = x_f[r] - o[r], row D = 1.0.  Columns of failed frames and of padding, rows of padding: ZEROS --
//                  neutral, bit for bit, in f64 sums that start at +0.0 -- so the product carries no per-frame condition.  A workgroup
//                  transposes a tile of 64 rows x 64 frames through LDS: lanes along the rows when reading the slots, along the frames when writing.
//   k_cv_product   Q += P P^T on v_mfma_f64_16x16x4_f64, a symmetric rank-K update.  One workgroup (4 waves) per block of Q with block-row
//                  <= block-column; blocks below the diagonal are never enumerated.  Wave (wr, wc) OWNS the 32 x 32 quarter of the block
//                  (2 x 2 tiles): it loads the stored values as its accumulators, walks the segment's trips in ascending order -- a trip is
//                  GR_CV_TRIP = 16 frames: a lane fetches one float4 per operand row (frames 16 g + 4 (lane >> 4) + j; lane & 15 = the row of
//                  the tile), MFMA j of the trip takes element j of every lane -- and stores them back.  Operands come straight from the
//                  panel (L2 / L1: a block's 128 operand rows of a trip are 8 KiB), the next trip's requested before this trip's MFMAs.
// ORDER OF THE SUMS: every entry of Q belongs to ONE wave and is ONE chain of MFMAs over the trips; frames are not split over waves, nothing
// is added in LDS or HBM, no atomic touches Q.  So the bits of Q are a function of the SEQUENCE OF CALLS (their frames and where the calls
// cut them) alone -- not of the grid, gr_covar_set_launch, the context's history or the run.  A diagonal block computes (i, j) and (j, i)
// from the same operands in the same order: Q is exactly symmetric.  NOT guaranteed: the same bits for different cuts of the same frames
// into calls (one MFMA adds four frames in an order the hardware does not document) -- that holds to the rounding bound only.
// STORAGE of a block: in accumulator order, double [wave][tile a][tile b][q][lane] -- every load and store of a wave is one contiguous
// 512-byte row; cv_at() is the host's map from (i, j) to it.
#pragma once
#include "gr_fluct.h"

#if defined(__HIPCC__)

#define GR_CV_BLOCK 64u                   /* edge of a block of Q, in dimensions */
#define GR_CV_TRIP 16u                    /* frames per trip of the product: one float4 per lane and operand row, four MFMAs */
#define GR_CV_BLOCK_LEN (GR_CV_BLOCK * GR_CV_BLOCK)
#define GR_CV_PACK_LD 65u                 /* floats per row of the pack tile in LDS (odd: the transposed reads spread over the banks) */

struct gr_covar {
    gr_ctx *c = nullptr;
    std::string group;
    GrSnapshot snap;                      // the group's atoms at create
    GrVerdicts verdicts;
    std::vector<float> masses;            // of the snapshot's atoms at create (the closing step's only)
    uint32_t n_atoms = 0;
    uint32_t D = 0, R = 0, rpad = 0, nblk = 0;        // dimensions, rows of the product (D + 1), ... rounded up to the block, block rows
    uint64_t ntri = 0;                    // blocks stored: nblk (nblk + 1) / 2
    grbuf::Dev<float> o, panel;           // [rpad], [rpad][GR_MAX_BATCH]
    grbuf::Dev<double> Q;                 // [ntri][GR_CV_BLOCK_LEN]
    grbuf::Pinned<double> q_host;         // cv_get's copy of Q.  Pinned and kept: a pageable block of this size is registered with the driver for
                                          // the copy, and freeing it right after makes the driver evict the process's queues -- the next launch of
                                          // the context then waits some 20 ms for their restore (seen as a resident pass that misses its poll)
    uint64_t n = 0;                      // counted frames
    uint32_t product_groups = 0, check_groups = 0;    // gr_covar_set_launch; 0: the default
    uint32_t last_product = 0, last_check = 0;        // grids of the last segment that was launched
    uint64_t launches = 0;
};

typedef double gr_cv_d4 __attribute__((ext_vector_type(4)));

namespace {

// row r of the product: dimension r of the snapshot (r < D), the ones row (r == D) or padding
__device__ __forceinline__ uint32_t cv_row_offset(const uint32_t *__restrict__ atoms, uint32_t r) { return (uint32_t)gr_tile_index(atoms[r / 3u], (int)(r % 3u)); }

__global__ __launch_bounds__(256) void k_cv_origin(const float *__restrict__ frames, size_t stride, uint32_t s0, uint32_t nf, const uint32_t *__restrict__ atoms, uint32_t D,
                                                   const uint32_t *__restrict__ verdict, float *__restrict__ o) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    uint32_t f = 0;
    while (f < nf && verdict[f] != GR_NOIDX) ++f;          // (the same in every lane)
    if (f == nf || r >= D) return;
    o[r] = frames[(size_t)(s0 + f) * stride + cv_row_offset(atoms, r)];
}

// block (x, y): rows 64 x .. 64 x + 63 (rpad is a multiple of 64), frames 64 y .. 64 y + 63 of the segment, those below kpad
__global__ __launch_bounds__(256) void k_cv_pack(const float *__restrict__ frames, size_t stride, uint32_t s0, uint32_t nf, uint32_t kpad, const uint32_t *__restrict__ atoms,
                                                 uint32_t D, const uint32_t *__restrict__ verdict, const float *__restrict__ o, float *__restrict__ P) {
    __shared__ float tile[64u * GR_CV_PACK_LD];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t r = blockIdx.x * 64u + lane, f0 = blockIdx.y * 64u;
    const uint32_t off = r < D ? cv_row_offset(atoms, r) : 0u;
    const float org = r < D ? o[r] : 0.0f;
    for (uint32_t k = 0; k < 16u; ++k) {
        const uint32_t fl = 16u * wave + k, f = f0 + fl;
        float v = 0.0f;
        if (f < nf && verdict[f] == GR_NOIDX) {            // (the same in every lane)
            if (r < D) v = frames[(size_t)(s0 + f) * stride + off] - org;
            else if (r == D) v = 1.0f;
        }
        tile[lane * GR_CV_PACK_LD + fl] = v;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t at = threadIdx.x + 256u * k, row = at >> 4, fq = at & 15u;
        if (f0 + 4u * fq >= kpad) continue;                // (kpad is a multiple of 16: a quad lies wholly inside or outside)
        const float *t = tile + row * GR_CV_PACK_LD + 4u * fq;
        *reinterpret_cast<float4 *>(P + (size_t)(blockIdx.x * 64u + row) * kpad + f0 + 4u * fq) = make_float4(t[0], t[1], t[2], t[3]);
    }
}

// the upper block triangle in row order: block t = (bi, bj), bi <= bj
__global__ __launch_bounds__(256) void k_cv_product(const float *__restrict__ P, uint32_t kpad, uint32_t nblk, uint32_t ntri, double *__restrict__ Q) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, m = lane & 15u, kg = lane >> 4;
    const uint32_t wr = wave >> 1, wc = wave & 1u;
    const uint32_t trips = kpad / GR_CV_TRIP;
    for (uint32_t t = blockIdx.x; t < ntri; t += gridDim.x) {
        uint32_t bi = 0, rem = t;
        while (rem >= nblk - bi) { rem -= nblk - bi; ++bi; }
        const uint32_t bj = bi + rem;
        // operand rows of this lane: tile a of A holds rows 64 bi + 32 wr + 16 a + m, tile b of B rows 64 bj + 32 wc + 16 b + m of the panel
        const float *pa[2], *pb[2];
#pragma unroll
        for (uint32_t a = 0; a < 2u; ++a) {
            pa[a] = P + (size_t)(GR_CV_BLOCK * bi + 32u * wr + 16u * a + m) * kpad + 4u * kg;
            pb[a] = P + (size_t)(GR_CV_BLOCK * bj + 32u * wc + 16u * a + m) * kpad + 4u * kg;
        }
        // C/D map of the f64 form: lane holds column lane & 15, rows (lane >> 4) + 4 q of its tile
        double *Qw = Q + (size_t)t * GR_CV_BLOCK_LEN + (size_t)wave * (GR_CV_BLOCK_LEN / 4u) + lane;
        gr_cv_d4 acc[2][2];
#pragma unroll
        for (uint32_t a = 0; a < 2u; ++a)
#pragma unroll
            for (uint32_t b = 0; b < 2u; ++b)
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q) acc[a][b][q] = Qw[((2u * a + b) * 4u + q) * 64u];
        float4 a4[2], b4[2];
#pragma unroll
        for (uint32_t a = 0; a < 2u; ++a) { a4[a] = *reinterpret_cast<const float4 *>(pa[a]); b4[a] = *reinterpret_cast<const float4 *>(pb[a]); }
        for (uint32_t g = 0; g < trips; ++g) {
            const float av[2][4] = { { a4[0].x, a4[0].y, a4[0].z, a4[0].w }, { a4[1].x, a4[1].y, a4[1].z, a4[1].w } };
            const float bv[2][4] = { { b4[0].x, b4[0].y, b4[0].z, b4[0].w }, { b4[1].x, b4[1].y, b4[1].z, b4[1].w } };
            // the next trip's operands (behind the last trip: the last trip's again, never used)
            const size_t next = (size_t)min(g + 1u, trips - 1u) * GR_CV_TRIP;
#pragma unroll
            for (uint32_t a = 0; a < 2u; ++a) { a4[a] = *reinterpret_cast<const float4 *>(pa[a] + next); b4[a] = *reinterpret_cast<const float4 *>(pb[a] + next); }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av[a][j], (double)bv[b][j], acc[a][b], 0, 0, 0);
        }
#pragma unroll
        for (uint32_t a = 0; a < 2u; ++a)
#pragma unroll
            for (uint32_t b = 0; b < 2u; ++b)
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q) Qw[((2u * a + b) * 4u + q) * 64u] = acc[a][b][q];
    }
}

// where entry (i, j) of Q, block-row <= block-column, lies in the block storage (the accumulator order of k_cv_product)
size_t cv_at(const gr_covar *f, uint32_t i, uint32_t j) {
    const uint32_t bi = i / GR_CV_BLOCK, bj = j / GR_CV_BLOCK, li = i % GR_CV_BLOCK, lj = j % GR_CV_BLOCK;
    const size_t blk = (size_t)bi * f->nblk - ((size_t)bi * bi - bi) / 2u + (bj - bi);      // rows 0 .. bi - 1 hold nblk, nblk - 1, ... blocks
    const uint32_t wave = 2u * (li / 32u) + lj / 32u, tile = 2u * ((li % 32u) / 16u) + (lj % 32u) / 16u, rr = li % 16u;
    return blk * GR_CV_BLOCK_LEN + (size_t)((wave * 4u + tile) * 4u + rr / 4u) * 64u + (rr % 4u) * 16u + lj % 16u;
}
size_t cv_q_len(const gr_covar *f) { return (size_t)f->ntri * GR_CV_BLOCK_LEN; }

// the state in group order: o [D], s [D] (column D of the product), Q [D][D] as the full square (a block below the diagonal is the
// mirror of the one above; a diagonal block is read as the device computed it, both triangles); each may be null
int cv_get(gr_covar *f, float *o, double *s, double *Q) {
    gr_ctx *c = f->c;
    (void)hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (o) HIPCHK(c, hipMemcpy(o, f->o.get(), (size_t)f->D * sizeof(float), hipMemcpyDeviceToHost));
    if (!s && !Q) return GR_OK;
    HIPCHK(c, f->q_host.reserve(cv_q_len(f), grbuf::exact));
    const double *q = f->q_host.get();
    HIPCHK(c, hipMemcpy(f->q_host.get(), f->Q.get(), cv_q_len(f) * sizeof(double), hipMemcpyDeviceToHost));
    const uint32_t D = f->D;
    if (s) for (uint32_t i = 0; i < D; ++i) s[i] = q[cv_at(f, i, D)];
    if (Q)
        for (uint32_t i = 0; i < D; ++i)
            for (uint32_t j = 0; j < D; ++j) Q[(size_t)i * D + j] = i / GR_CV_BLOCK <= j / GR_CV_BLOCK ? q[cv_at(f, i, j)] : q[cv_at(f, j, i)];
    return GR_OK;
}

// ... and back, with n counted frames (rows and columns of padding are zero, as the kernel keeps them)
int cv_put(gr_covar *f, const float *o, const double *s, const double *Q, uint64_t n) {
    gr_ctx *c = f->c;
    (void)hipSetDevice(c->device);
    std::vector<double> q(cv_q_len(f), 0.0);
    const uint32_t D = f->D;
    for (uint32_t i = 0; i < D; ++i) {
        for (uint32_t j = 0; j < D; ++j)
            if (i / GR_CV_BLOCK <= j / GR_CV_BLOCK) q[cv_at(f, i, j)] = Q[(size_t)i * D + j];
        q[cv_at(f, i, D)] = s[i];
        if (i / GR_CV_BLOCK == D / GR_CV_BLOCK) q[cv_at(f, D, i)] = s[i];
    }
    q[cv_at(f, D, D)] = (double)n;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(f->o.get(), o, (size_t)D * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(f->Q.get(), q.data(), q.size() * sizeof(double), hipMemcpyHostToDevice));
    f->n = n;
    return GR_OK;
}

int cv_zero(gr_covar *f) {
    gr_ctx *c = f->c;
    HIPCHK(c, hipMemsetAsync(f->o.get(), 0, (size_t)f->rpad * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(f->Q.get(), 0, cv_q_len(f) * sizeof(double), c->stream));
    f->n = 0;
    return GR_OK;
}

// the closing formulas on the host: mean [D] and cov [D][D] (in: Q, out: the covariance) of n counted frames; each may be null
void cv_close(const gr_covar *f, const float *o, const double *s, uint64_t n, double *mean, double *cov, bool weighted) {
    const size_t D = f->D;
    if (n == 0) {
        if (mean) std::fill(mean, mean + D, (double)NAN);
        if (cov) std::fill(cov, cov + D * D, (double)NAN);
        return;
    }
    const double dn = (double)n;
    if (mean) for (size_t i = 0; i < D; ++i) mean[i] = (double)o[i] + s[i] / dn;
    if (!cov) return;
    std::vector<double> rm(D, 1.0);
    if (weighted) for (size_t i = 0; i < D; ++i) rm[i] = sqrt((double)f->masses[i / 3]);
    for (size_t i = 0; i < D; ++i)
        for (size_t j = 0; j < D; ++j) {
            double v = (cov[i * D + j] - s[i] * s[j] / dn) / dn;
            if (weighted) v *= rm[i] * rm[j];
            cov[i * D + j] = v;
        }
}

int cv_accumulate(gr_covar *f, uint32_t first_slot, uint32_t n_frames, int *status_out) {
    gr_ctx *c = f->c;
    int st = slot_check(c, first_slot, n_frames); if (st) return st;
    (void)hipSetDevice(c->device);
    GrVerdicts &V = f->verdicts;
    const uint32_t *vd = V.dev.get(), *atoms = f->snap.atoms_dev.get();
    grb::FirstError<gr_ctx> fe;
    for (const auto [b0, nb, s0] : grb::Segments{ first_slot, n_frames }) {
        const grb::Prechecks pre(c, { b0, nb, s0 }, box_checks(c, false));
        if (pre.any_ok) {
            SlotUse use(c, s0, nb);
            st = V.begin(c, pre, nb); if (st) return st;
            // launch geometry: one workgroup per stored block of Q; gr_covar_set_launch caps both grids
            const uint32_t kpad = (nb + GR_CV_TRIP - 1u) & ~(GR_CV_TRIP - 1u);
            uint32_t product = (uint32_t)f->ntri;
            if (f->product_groups && f->product_groups < product) product = f->product_groups;
            const uint32_t check = V.check(c, f->snap, s0, nb, f->check_groups);
            if (f->n == 0) k_cv_origin<<<dim3((f->D + 255u) / 256u), dim3(256), 0, c->stream>>>(c->frames, c->frame_stride, s0, nb, atoms, f->D, vd, f->o.get());
            k_cv_pack<<<dim3(f->rpad / 64u, (kpad + 63u) / 64u), dim3(256), 0, c->stream>>>(c->frames, c->frame_stride, s0, nb, kpad, atoms, f->D, vd, f->o.get(), f->panel.get());
            k_cv_product<<<dim3(product), dim3(256), 0, c->stream>>>(f->panel.get(), kpad, f->nblk, (uint32_t)f->ntri, f->Q.get());
            HIPCHK(c, hipGetLastError());
            ++f->launches; f->last_product = product; f->last_check = check;
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

gr_covar *gr_covar_create(gr_ctx *c, const char *group, int *status) try {
    int dummy; if (!status) status = &dummy;
    if (!c) { *status = GR_E_INVALID_ARG; return nullptr; }
    *status = busy_check(c); if (*status) return nullptr;
    const Group *g = need_group(c, group, *status, true); if (!g) return nullptr;
    std::unique_ptr<gr_covar> f(new gr_covar());
    f->c = c; f->group = group;
    std::vector<uint32_t> atoms = hb_group_atoms(*g);
    if (atoms.size() > GR_CV_MAX_ATOMS) {
        *status = fail(c, GR_E_INVALID_ARG, "covariance: the group has more than GR_CV_MAX_ATOMS = " + std::to_string(GR_CV_MAX_ATOMS) + " atoms");
        return nullptr;
    }
    f->n_atoms = (uint32_t)atoms.size();
    for (uint32_t a : atoms) f->masses.push_back(c->masses_host[a]);
    f->D = 3u * f->n_atoms; f->R = f->D + 1u;
    f->rpad = (f->R + GR_CV_BLOCK - 1u) & ~(GR_CV_BLOCK - 1u);
    f->nblk = f->rpad / GR_CV_BLOCK;
    f->ntri = (uint64_t)f->nblk * (f->nblk + 1u) / 2u;
    (void)hipSetDevice(c->device);
    bool ok = f->snap.build(c, std::move(atoms)) && f->verdicts.reserve(0u) && f->o.reserve(f->rpad, grbuf::exact) == hipSuccess &&
              f->panel.reserve((size_t)f->rpad * GR_MAX_BATCH, grbuf::exact) == hipSuccess && f->Q.reserve(cv_q_len(f.get()), grbuf::exact) == hipSuccess;
    ok = ok && cv_zero(f.get()) == GR_OK && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        *status = fail(c, GR_E_HIP, "covariance: device allocation failed");
        return nullptr;
    }
    *status = GR_OK;
    return f.release();
} catch (...) { if (status) *status = gr_abi_guard(); return nullptr; }

void gr_covar_destroy(gr_covar *f) try { gr_object_destroy(f); } catch (...) { }

int gr_covar_accumulate_batch(gr_covar *f, uint32_t first_slot, uint32_t n_frames, int *status_out) try {
    if (!f) return GR_E_INVALID_ARG;
    return cv_accumulate(f, first_slot, n_frames, status_out);
} catch (...) { return gr_abi_guard(); }

int gr_covar_clear(gr_covar *f) try {
    if (!f) return GR_E_INVALID_ARG;
    int st = busy_check(f->c); if (st) return st;
    (void)hipSetDevice(f->c->device);
    return cv_zero(f);
} catch (...) { return gr_abi_guard(); }

uint64_t gr_covar_frames(const gr_covar *f) { return f ? f->n : 0u; }
uint64_t gr_covar_n_atoms(const gr_covar *f) { return f ? f->n_atoms : 0u; }

int gr_covar_read_raw(gr_covar *f, float *origin, double *sum, double *Q, uint64_t *n) try {
    if (!f) return GR_E_INVALID_ARG;
    int st = busy_check(f->c); if (st) return st;
    if (origin || sum || Q) { st = cv_get(f, origin, sum, Q); if (st) return st; }
    if (n) *n = f->n;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_covar_read(gr_covar *f, double *mean, double *cov, uint32_t flags) try {
    if (!f) return GR_E_INVALID_ARG;
    int st = busy_check(f->c); if (st) return st;
    if (flags & ~(uint32_t)GR_CV_MASS_WEIGHTED) return fail(f->c, GR_E_INVALID_ARG, "covariance: unknown flags");
    std::vector<float> o(f->D); std::vector<double> s(f->D);
    st = cv_get(f, o.data(), s.data(), cov); if (st) return st;
    cv_close(f, o.data(), s.data(), f->n, mean, cov, (flags & GR_CV_MASS_WEIGHTED) != 0u);
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_covar_read_dccm(gr_covar *f, double *corr) try {
    if (!f || !corr) return GR_E_INVALID_ARG;
    int st = busy_check(f->c); if (st) return st;
    const size_t D = f->D, S = f->n_atoms;
    std::vector<float> o(D); std::vector<double> s(D), cov(D * D);
    st = cv_get(f, o.data(), s.data(), cov.data()); if (st) return st;
    cv_close(f, o.data(), s.data(), f->n, nullptr, cov.data(), false);
    std::vector<double> tr(S);
    for (size_t a = 0; a < S; ++a) tr[a] = cov[(3 * a) * D + 3 * a] + cov[(3 * a + 1) * D + 3 * a + 1] + cov[(3 * a + 2) * D + 3 * a + 2];
    for (size_t a = 0; a < S; ++a)
        for (size_t b = 0; b < S; ++b) {
            if (f->n == 0) { corr[a * S + b] = NAN; continue; }
            if (!(tr[a] > 0.0) || !(tr[b] > 0.0)) { corr[a * S + b] = a == b ? 1.0 : (double)NAN; continue; }       // an atom that does not move
            const double x = cov[(3 * a) * D + 3 * b] + cov[(3 * a + 1) * D + 3 * b + 1] + cov[(3 * a + 2) * D + 3 * b + 2];
            corr[a * S + b] = x / sqrt(tr[a] * tr[b]);
        }
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_covar_merge(gr_covar *dst, gr_covar *src) try {
    if (!dst || !src) return GR_E_INVALID_ARG;
    gr_ctx *c = dst->c;
    int st = busy_check(c); if (st) return st;
    if (src->c != c) { st = busy_check(src->c); if (st) return fail(c, st, src->c->err); }
    if (dst->n_atoms != src->n_atoms) { c->counts[0] = dst->n_atoms; c->counts[1] = src->n_atoms; return fail(c, GR_E_INCONSISTENT_GROUP, dst->group); }
    if (src == dst) return fail(c, GR_E_INVALID_ARG, "covariance: an object cannot be merged into itself");
    if (src->n == 0) return GR_OK;
    const size_t D = dst->D;
    std::vector<float> os(D), od(D); std::vector<double> ss(D), sd(D), Qs(D * D), Qd;
    st = cv_get(src, os.data(), ss.data(), Qs.data()); if (st) return src->c == c ? st : fail(c, st, src->c->err);
    if (dst->n == 0) return cv_put(dst, os.data(), ss.data(), Qs.data(), src->n);      // an empty object takes the other's origin and sums as they are
    Qd.resize(D * D);
    st = cv_get(dst, od.data(), sd.data(), Qd.data()); if (st) return st;
    // src's sums moved to dst's origin: d' = d + delta with delta = o_src - o_dst (the upper triangle, mirrored: Q stays exactly symmetric)
    const double ns = (double)src->n;
    std::vector<double> delta(D);
    for (size_t i = 0; i < D; ++i) delta[i] = (double)os[i] - (double)od[i];
    for (size_t i = 0; i < D; ++i)
        for (size_t j = i; j < D; ++j) {
            Qd[i * D + j] += Qs[i * D + j] + delta[i] * ss[j] + ss[i] * delta[j] + ns * delta[i] * delta[j];
            Qd[j * D + i] = Qd[i * D + j];
        }
    for (size_t i = 0; i < D; ++i) sd[i] += ss[i] + ns * delta[i];
    return cv_put(dst, od.data(), sd.data(), Qd.data(), dst->n + src->n);
} catch (...) { return gr_abi_guard(); }

int gr_covar_set_launch(gr_covar *f, uint32_t product_groups, uint32_t check_groups) try {
    if (!f) return GR_E_INVALID_ARG;
    f->product_groups = product_groups; f->check_groups = check_groups;
    return GR_OK;
} catch (...) { return gr_abi_guard(); }

int gr_covar_stat(const gr_covar *f, int key, uint64_t *value) try {
    if (!f || !value) return GR_E_INVALID_ARG;
    switch (key) {
    case GR_CV_STAT_LAUNCHES: *value = f->launches; return GR_OK;
    case GR_CV_STAT_LAST_PRODUCT_GROUPS: *value = f->last_product; return GR_OK;
    case GR_CV_STAT_LAST_CHECK_GROUPS: *value = f->last_check; return GR_OK;
    case GR_CV_STAT_BLOCK_EDGE: *value = GR_CV_BLOCK; return GR_OK;
    case GR_CV_STAT_TRIP_FRAMES: *value = GR_CV_TRIP; return GR_OK;
    case GR_CV_STAT_BLOCKS: *value = f->ntri; return GR_OK;
    default: return GR_E_INVALID_ARG;
    }
} catch (...) { return gr_abi_guard(); }

}  // extern "C"

#endif  // __HIPCC__
