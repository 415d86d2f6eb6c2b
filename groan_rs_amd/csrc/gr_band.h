// gr_band.h -- the BAND PRODUCT that MSD (gr_msd.h) and VectorCorrelation (gr_vcorr.h) share: the sums, per lag tau <= max_lag, of a
// function of G = X X^T over the frame pairs (t, t + tau) of a panel X[T][K] (f32, one row per frame), and the integer geometry of the
// band, which the host and the kernels take from the same functions.
//
// GEOMETRY (no HIP in this half: tests/test_band_host.py compiles it with the host compiler).  G is cut into 64 x 64 blocks of frame
// pairs; only the blocks with block-row <= block-column that touch the band t' - t <= max_lag are enumerated: block row bi holds the
// block columns bi .. min(bi + W, nblk - 1).  Rows 0 .. r0 - 1 (r0 = nblk - W) hold W + 1 blocks, row bi >= r0 holds nblk - bi; the
// blocks are numbered row by row (block_index and block_decode are inverses).  The pair counts are integer work on the ok flags.
//   k_band_gram<DIST>  G on v_mfma_f64_16x16x4_f64 (widened f32 operands: exact products, f64 sums), one workgroup of four waves per
//                 block as in k_cv_product: wave (wr, wc) owns a 32 x 32 quarter (2 x 2 tiles); the contraction runs over the K values
//                 of a row in trips of GR_BAND_TRIP = 16, ascending, operands straight from the panel (L2 / L1), GR_BAND_AHEAD trips in
//                 flight (K / GR_BAND_TRIP = 4 C n_pad / 64 with C = 3 or 6 components is a multiple of GR_BAND_AHEAD = 3: the loop has
//                 no tail).  Every entry belongs to ONE wave and is ONE chain of MFMAs: its bits depend on its two rows and K alone.
//                 blockIdx.y is the panel: one launch serves up to two.  The block's value for a valid pair (ok on both sides,
//                 t' - t <= max_lag) goes to LDS and 127 lanes add one diagonal of the block each, rows ascending: the per-diagonal
//                 partial sums of the block.
//                 DIST = true   D2 = (q_t + q_t') - 2 G with q the rows' squared norms; valid pairs have t < t' (D2(t, t) IS DEFINED AS 0:
//                               the chain of G(t, t) and the sum behind q_t are two orders of the same sum and differ by rounding)
//                 DIST = false  G itself; the diagonal t = t' is a valid pair (lag 0)
//   k_band_lags   one lane per lag: the partials of that lag in ascending block-row order (per block row: the nearer block column first).
// No atomic decides a sum; sum[tau] is a function of the panel (and so a prefix of the full curve's for any max_lag).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#define GR_BAND_BLOCK 64u                 /* edge of a block of the Gram matrix, in frames */
#define GR_BAND_TRIP 16u                  /* panel values per trip of the product: one float4 per lane and operand row, four MFMAs */
#define GR_BAND_AHEAD 3u                  /* trips whose operands a wave of the product has in flight */
#define GR_BAND_DIAGS (2u * GR_BAND_BLOCK - 1u)    /* diagonals of a block: t' - t = -63 .. 63 inside it */
#define GR_BAND_LD (GR_BAND_BLOCK + 1u)   /* doubles per row of the block in LDS (odd: a diagonal's lanes read consecutive banks) */

#if defined(__HIPCC__)
#define GR_BAND_FN __host__ __device__ __forceinline__
#else
#define GR_BAND_FN inline
#endif

namespace grband {

// block (bi, bi + db) -> its number
GR_BAND_FN uint32_t block_index(uint32_t bi, uint32_t db, uint32_t nblk, uint32_t W) {
    const uint32_t r0 = nblk - W;
    if (bi < r0) return bi * (W + 1u) + db;
    const uint32_t k = bi - r0;           // short rows in front of this one: W, W - 1, ... blocks
    return r0 * (W + 1u) + k * W - (k * (k - 1u)) / 2u + db;
}

// ... and back
GR_BAND_FN void block_decode(uint32_t t, uint32_t nblk, uint32_t W, uint32_t &bi, uint32_t &db) {
    const uint32_t r0 = nblk - W;
    if (t < r0 * (W + 1u)) { bi = t / (W + 1u); db = t % (W + 1u); }
    else {
        uint32_t rem = t - r0 * (W + 1u);
        bi = r0;
        while (rem >= nblk - bi) { rem -= nblk - bi; ++bi; }
        db = rem;
    }
}

// the band of T >= 1 frames: max_lag CLAMPED to T - 1 (a lag beyond the last frame has no pair), lags = max_lag + 1, nblk block rows,
// W = the farthest block column of a row, nblocks blocks in all
struct Geometry { uint32_t max_lag, lags, nblk, W; uint64_t nblocks; };

inline Geometry geometry(uint32_t T, uint32_t max_lag) {
    Geometry g;
    g.max_lag = std::min(max_lag, T - 1u);
    g.lags = g.max_lag + 1u;
    g.nblk = (T + GR_BAND_BLOCK - 1u) / GR_BAND_BLOCK;
    g.W = std::min(g.nblk - 1u, (g.max_lag + GR_BAND_BLOCK - 1u) / GR_BAND_BLOCK);
    g.nblocks = (uint64_t)(g.nblk - g.W) * (g.W + 1u) + (uint64_t)g.W * (g.W + 1u) / 2u;
    return g;
}

// pairs[tau] = the t with ok[t] and ok[t + tau], tau < lags
inline void pair_counts(const uint8_t *ok, uint32_t T, uint32_t lags, std::vector<uint64_t> &pairs) {
    pairs.assign(lags, 0u);
    for (uint32_t tau = 0; tau < lags; ++tau) {
        uint64_t n = 0;
        for (uint32_t t = 0; t + tau < T; ++t) n += (uint64_t)(ok[t] & ok[t + tau]);
        pairs[tau] = n;
    }
}

}  // namespace grband

#if defined(__HIPCC__)

typedef double gr_band_d4 __attribute__((ext_vector_type(4)));

namespace {

// block t of the band of panel blockIdx.y -> part[blockIdx.y][t][GR_BAND_DIAGS]; T frames, Ka / Kb values per row of panel 0 / 1 (a
// multiple of GR_BAND_TRIP * GR_BAND_AHEAD), ok[T] and q[T] (DIST only) per frame, nblocks < 2^31.  DIST has ONE panel (gridDim.y = 1):
// there the choice of the panel is compiled out, it would cost scalar registers and a longer prologue for nothing
template <bool DIST>
__global__ __launch_bounds__(256) void k_band_gram(const float *__restrict__ Xa, uint32_t Ka, const float *__restrict__ Xb, uint32_t Kb, const uint32_t *__restrict__ ok,
                                                   uint32_t T, uint32_t nblk, uint32_t W, uint32_t nblocks, uint32_t max_lag, double *__restrict__ part,
                                                   const double *__restrict__ q) {
    __shared__ double D[GR_BAND_BLOCK * GR_BAND_LD];
    const bool second = !DIST && blockIdx.y != 0u;
    const float *__restrict__ X = second ? Xb : Xa;
    const uint32_t K = second ? Kb : Ka;
    if (!DIST) part += (size_t)blockIdx.y * nblocks * GR_BAND_DIAGS;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, m = lane & 15u, kg = lane >> 4;
    const uint32_t wr = wave >> 1, wc = wave & 1u;
    const uint32_t trips = K / GR_BAND_TRIP;
    for (uint32_t t = blockIdx.x; t < nblocks; t += gridDim.x) {
        uint32_t bi, db;
        grband::block_decode(t, nblk, W, bi, db);
        const uint32_t bj = bi + db;
        gr_band_d4 acc[2][2];
#pragma unroll
        for (uint32_t a = 0; a < 2u; ++a)
#pragma unroll
            for (uint32_t b = 0; b < 2u; ++b) acc[a][b] = (gr_band_d4){ 0.0, 0.0, 0.0, 0.0 };
        // (the quarter below the diagonal of a diagonal block holds no valid pair: its wave waits)
        if (!(bi == bj && wr > wc)) {
            // operand rows of this lane: tile a of A holds frames 64 bi + 32 wr + 16 a + m, tile b of B frames 64 bj + 32 wc + 16 b + m; a frame
            // beyond the panel's last is read as the last (never closed)
            const float *pa[2], *pb[2];
#pragma unroll
            for (uint32_t a = 0; a < 2u; ++a) {
                pa[a] = X + (size_t)min(GR_BAND_BLOCK * bi + 32u * wr + 16u * a + m, T - 1u) * K + 4u * kg;
                pb[a] = X + (size_t)min(GR_BAND_BLOCK * bj + 32u * wc + 16u * a + m, T - 1u) * K + 4u * kg;
            }
            // the operands of GR_BAND_AHEAD trips are in flight (behind the last trip: the last trip's again, never used); the MFMAs keep
            // the ascending order of the trips
            float4 a4[GR_BAND_AHEAD][2], b4[GR_BAND_AHEAD][2];
#pragma unroll
            for (uint32_t p = 0; p < GR_BAND_AHEAD; ++p) {
                const size_t at = (size_t)min(p, trips - 1u) * GR_BAND_TRIP;
#pragma unroll
                for (uint32_t a = 0; a < 2u; ++a) { a4[p][a] = *reinterpret_cast<const float4 *>(pa[a] + at); b4[p][a] = *reinterpret_cast<const float4 *>(pb[a] + at); }
            }
            for (uint32_t g0 = 0; g0 < trips; g0 += GR_BAND_AHEAD) {
#pragma unroll
                for (uint32_t p = 0; p < GR_BAND_AHEAD; ++p) {
                    const uint32_t g = g0 + p;
                    if (g >= trips) break;                          // (the same in every lane and never taken, see `trips`; without it the accumulators move between AGPRs and VGPRs every turn)
                    const float av[2][4] = { { a4[p][0].x, a4[p][0].y, a4[p][0].z, a4[p][0].w }, { a4[p][1].x, a4[p][1].y, a4[p][1].z, a4[p][1].w } };
                    const float bv[2][4] = { { b4[p][0].x, b4[p][0].y, b4[p][0].z, b4[p][0].w }, { b4[p][1].x, b4[p][1].y, b4[p][1].z, b4[p][1].w } };
                    const size_t next = (size_t)min(g + GR_BAND_AHEAD, trips - 1u) * GR_BAND_TRIP;
#pragma unroll
                    for (uint32_t a = 0; a < 2u; ++a) { a4[p][a] = *reinterpret_cast<const float4 *>(pa[a] + next); b4[p][a] = *reinterpret_cast<const float4 *>(pb[a] + next); }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int a = 0; a < 2; ++a)
#pragma unroll
                            for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av[a][j], (double)bv[b][j], acc[a][b], 0, 0, 0);
                }
            }
        }
        // C/D map of the f64 form: lane holds column lane & 15, rows (lane >> 4) + 4 p of its tile
#pragma unroll
        for (uint32_t a = 0; a < 2u; ++a)
#pragma unroll
            for (uint32_t b = 0; b < 2u; ++b) {
                const uint32_t j = 32u * wc + 16u * b + m, gj = GR_BAND_BLOCK * bj + j, cj = min(gj, T - 1u);
                const double qj = DIST ? q[cj] : 0.0;
                const bool okj = gj < T && ok[cj] != 0u;
#pragma unroll
                for (uint32_t p = 0; p < 4u; ++p) {
                    const uint32_t i = 32u * wr + 16u * a + kg + 4u * p, gi = GR_BAND_BLOCK * bi + i, ci = min(gi, T - 1u);
                    const bool valid = okj && (DIST ? gi < gj : gi <= gj) && gj - gi <= max_lag && ok[ci] != 0u;
                    if (DIST) D[i * GR_BAND_LD + j] = valid ? (q[ci] + qj) - 2.0 * acc[a][b][p] : 0.0;
                    else D[i * GR_BAND_LD + j] = valid ? acc[a][b][p] : 0.0;
                }
            }
        __syncthreads();
        if (threadIdx.x < GR_BAND_DIAGS) {
            // diagonal j - i = threadIdx.x - 63 of the block, rows ascending
            const uint32_t dl = threadIdx.x;
            const uint32_t i0 = dl < GR_BAND_BLOCK - 1u ? GR_BAND_BLOCK - 1u - dl : 0u, i1 = dl > GR_BAND_BLOCK - 1u ? GR_BAND_DIAGS - dl : GR_BAND_BLOCK;
            double s = 0.0;
            for (uint32_t i = i0; i < i1; ++i) s += D[i * GR_BAND_LD + i + dl - (GR_BAND_BLOCK - 1u)];
            part[(size_t)t * GR_BAND_DIAGS + dl] = s;
        }
        __syncthreads();
    }
}

// lag tau = 64 d0 + r: diagonal r of the blocks (bi, bi + d0) and diagonal r - 64 of the blocks (bi, bi + d0 + 1), block rows ascending
__global__ __launch_bounds__(256) void k_band_lags(const double *__restrict__ part, uint32_t nblk, uint32_t W, uint32_t lags, double *__restrict__ sums) {
    const uint32_t tau = blockIdx.x * 256u + threadIdx.x;
    if (tau >= lags) return;
    const uint32_t d0 = tau / GR_BAND_BLOCK, r = tau % GR_BAND_BLOCK;
    double s = 0.0;
    for (uint32_t bi = 0; bi < nblk; ++bi) {
        if (d0 <= W && bi + d0 < nblk) s += part[(size_t)grband::block_index(bi, d0, nblk, W) * GR_BAND_DIAGS + (GR_BAND_BLOCK - 1u) + r];
        if (r >= 1u && d0 + 1u <= W && bi + d0 + 1u < nblk) s += part[(size_t)grband::block_index(bi, d0 + 1u, nblk, W) * GR_BAND_DIAGS + r - 1u];
    }
    sums[tau] = s;
}

// the scratch of an object's computes and what the last one launched
struct GrBandWork {
    grbuf::Dev<double> part, sums;        // [panels][blocks][GR_BAND_DIAGS], [panels][lags]
    uint32_t gram_groups = 0;             // the object's set_launch; 0: one workgroup per block
    uint32_t last_gram = 0;
    uint64_t blocks = 0;
};

// the band of T >= 1 frames and `panels` panels: its geometry and the scratch for it; `who` opens the messages ("msd", "vcorr")
int band_reserve(gr_ctx *c, const char *who, GrBandWork &w, uint32_t T, uint32_t max_lag, uint32_t panels, grband::Geometry &g) {
    g = grband::geometry(T, max_lag);
    if (g.nblocks > 0x7fffffffull) return fail(c, GR_E_INVALID_ARG, std::string(who) + ": too many blocks of frame pairs for one compute");
    if (w.part.reserve((size_t)panels * g.nblocks * GR_BAND_DIAGS, grbuf::exact) != hipSuccess || w.sums.reserve((size_t)panels * g.lags, grbuf::exact) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, GR_E_HIP, std::string(who) + ": device allocation failed");
    }
    return GR_OK;
}

// the product of panel 0 (and panel 1, if panels == 2) and the lag sums behind it: w.sums[p][lags].  Launch geometry: one workgroup per
// block and panel; gram_groups caps the grid along x
template <bool DIST>
int band_launch(gr_ctx *c, GrBandWork &w, const grband::Geometry &g, uint32_t panels, const float *Xa, uint32_t Ka, const float *Xb, uint32_t Kb, const double *q,
                 const uint32_t *ok, uint32_t T) {
    uint32_t grid = (uint32_t)g.nblocks;
    if (w.gram_groups && w.gram_groups < grid) grid = w.gram_groups;
    k_band_gram<DIST><<<dim3(grid, panels), dim3(256), 0, c->stream>>>(Xa, Ka, Xb, Kb, ok, T, g.nblk, g.W, (uint32_t)g.nblocks, g.max_lag, w.part.get(), q);
    for (uint32_t p = 0; p < panels; ++p)
        k_band_lags<<<dim3((g.lags + 255u) / 256u), dim3(256), 0, c->stream>>>(w.part.get() + (size_t)p * g.nblocks * GR_BAND_DIAGS, g.nblk, g.W, g.lags,
                                                                               w.sums.get() + (size_t)p * g.lags);
    HIPCHK(c, hipGetLastError());
    w.last_gram = grid; w.blocks = g.nblocks;
    return GR_OK;
}

}  // namespace

#endif  // __HIPCC__
