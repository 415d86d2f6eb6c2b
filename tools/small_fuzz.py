#!/usr/bin/env python3
"""Randomised soak of the single-wave kernels of one-frame calls (gr_small.h, GR_TUNE_SMALL_CALLS) on the GPU box: systems of 300 .. 20 000
atoms, selections of 1 .. 4 096 atoms drawn as one block or as scattered indices, three cells, blobs narrow enough for the image proof
or wide enough to fail it, an atom without position or without mass inside the selection now and then, the reference's masses its own
(drawn independently of the target's) in half of the cases.  Every call -- naive COM, Bai-Breen
estimate (centre and COM), get_center / get_com, group_distance of two groups, calc_rmsd, calc_rmsd_and_fit (one frame per call and as a
batch) -- is compared with the batched kernels (GR_TUNE_SMALL_CALLS = 0) on the same frames: the same error (variant and atom index) or
centres to 5e-6 nm, rmsd to 2e-6, rotations to the conditioning of their Kabsch problem and fitted coordinates to 1.5e-5 + |dR| x distance from
the group (the comment at the comparison says why a flat limit cannot be right); one frame per case against the oracle.  Prints one line per case; exit
status 1 on a mismatch.

    python tools/small_fuzz.py [seconds] [seed]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import groan_rs_amd as G
import oracle_lib as O

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
CELLS = [([7.0, 6.5, 6.0], [90.0, 90.0, 90.0]), ([7.0, 6.5, 6.0], [75.0, 80.0, 70.0]), ([6.5, 6.5, 6.5], [60.0, 60.0, 90.0])]
CENTRES = ("group_get_com_naive", "group_estimate_com", "group_estimate_center", "group_get_com", "group_get_center")


def draw_group(n, lo_n=1):
    size = int(min(n, 4096, max(lo_n, rng.integers(1, 4097) if rng.random() < 0.3 else rng.integers(1, 600))))
    if rng.random() < 0.5:
        a = int(rng.integers(0, n - size + 1))
        return ("block", np.arange(a, a + size))
    return ("scattered", np.sort(rng.choice(n, size, replace=False)))


def call(fn):
    try:
        return ("ok", fn())
    except G.GroanError as e:
        return ("err", (type(e).__name__, e.variant, e.detail))


def same(a, b, tol):
    if a[0] != b[0]:
        return False
    if a[0] == "err":
        return a[1] == b[1]
    return np.abs(np.asarray(a[1], np.float64) - np.asarray(b[1], np.float64)).max() <= tol


def resultant(pos, idx, box, mass=None):
    """shortest mean resultant of the Bai-Breen angles over the three axes (1 = a point, ~1 / sqrt(n) = spread over the whole cell): the
    condition number of the centre estimate -- and of everything that unwraps about it -- is its inverse"""
    b = np.asarray(box, np.float64)
    H = np.array([[b[0], b[5], b[7]], [0.0, b[1], b[8]], [0.0, 0.0, b[2]]])          # columns a, b, c (gro order: xx yy zz xy xz yx yz zx zy)
    f = np.linalg.solve(H, np.nan_to_num(pos[idx].astype(np.float64)).T).T
    w = np.ones(len(idx)) if mass is None else np.nan_to_num(mass[idx].astype(np.float64), nan=1.0)
    z = (w[:, None] * np.exp(2j * np.pi * f)).sum(0) / w.sum()
    return float(np.abs(z).min())


t_end = time.time() + budget
cases = bad = small_total = ill = 0
worst_dr = worst_xyz = 0.0
while time.time() < t_end:
    n = int(rng.integers(300, 20001))
    lengths, angles = CELLS[int(rng.integers(0, 3))]
    box = O.box_from_lengths_angles(lengths, angles)
    nf = int(rng.integers(1, 5))
    wide = rng.random() < 0.2                               # a blob wider than half the cell: the image proof fails, the frame is redone
    spread = float(rng.uniform(0.8, 1.6)) if wide else float(rng.uniform(0.15, 0.55))
    masses = rng.uniform(1.0, 16.0, n).astype(np.float32)
    kind_a, ia = draw_group(n)
    kind_b, ib = draw_group(n)
    frames = []
    for f in range(nf + 1):
        blob = rng.normal(0, spread, (n, 3)) + rng.uniform(0.1, 0.9, 3) * np.array(lengths)
        frames.append(O.wrap_atoms(blob.astype(np.float32), np.arange(n), box))
    poison = rng.random() < 0.25
    if poison:                                              # an atom of group a without position (frame 0) / without mass
        if rng.random() < 0.5: frames[0][int(rng.choice(ia))] = np.nan
        else: masses[int(rng.choice(ia))] = np.nan
    systems = []
    for small in (4096, 0):
        s = G.System(n, masses=masses, n_slots=nf + 1)
        for f in range(nf + 1):
            s.set_frame(frames[f], box, slot=f)
        s.group_create_from_indices("a", ia) if kind_a == "scattered" else s.group_create_from_ranges("a", [(int(ia[0]), int(ia[-1]))])
        s.group_create_from_indices("b", ib) if kind_b == "scattered" else s.group_create_from_ranges("b", [(int(ib[0]), int(ib[-1]))])
        s.set_tuning(small_calls=small)
        systems.append(s)
    S, B = systems
    # half of the cases: the reference carries masses of its own, so the plan's weights are not the target's masses (GrPlanDev::w_is_mass = 0:
    # the second weight load and the separate sums of w v, in the single-wave kernels as in the batched ones)
    own_w = rng.random() < 0.5
    ref_masses = rng.uniform(1.0, 16.0, n).astype(np.float32) if own_w else np.nan_to_num(masses, nan=1.0)
    ref = G.System(n, masses=ref_masses, box=box, positions=np.nan_to_num(frames[nf], nan=1.0))
    ref.group_create_from_indices("a", ia) if kind_a == "scattered" else ref.group_create_from_ranges("a", [(int(ia[0]), int(ia[-1]))])
    ok = True
    why = ""
    # A group spread over the whole cell has a short resultant: its centre estimate -- and the images every later step chooses about it --
    # turn on the last bits of the sums, in the reference's f32 loop as much as here.  Such a case (resultant < 0.05 on some axis in some
    # frame) proves nothing about either path and is counted, not compared.
    if min(min(resultant(frames[f], ia, box), resultant(frames[f], ia, box, masses), resultant(frames[f], ib, box)) for f in range(nf + 1)) < 0.05:
        ill += 1
        for x in (S, B, ref): x.close()
        continue
    for f in range(nf):
        for fn in CENTRES:
            ra, rb = call(lambda: getattr(S, fn)("a", slot=f)), call(lambda: getattr(B, fn)("a", slot=f))
            if not same(ra, rb, 5e-6): ok = False; why += " %s[%d] %r != %r" % (fn, f, ra, rb)
        ra, rb = call(lambda: S.group_distance("a", "b", G.Dimension.XYZ, slot=f)), call(lambda: B.group_distance("a", "b", G.Dimension.XYZ, slot=f))
        if not same(ra, rb, 5e-6): ok = False; why += " distance[%d] %r != %r" % (f, ra, rb)
    plans = []
    try:
        plans = [G.RMSDPlan(ref, x, "a") for x in (S, B)]
    except G.GroanError:
        plans = []                                          # (the reference group has no mass-weighted centre: nothing to compare)
    if plans:
        for f in range(nf):
            ra, rb = call(lambda: plans[0].rmsd(f, 1)[0][0]), call(lambda: plans[1].rmsd(f, 1)[0][0])
            if not same(ra, rb, 2e-6): ok = False; why += " rmsd[%d] %r != %r" % (f, ra, rb)
        ra, rb = call(lambda: plans[0].rmsd(0, nf, raise_on_error=False)), call(lambda: plans[1].rmsd(0, nf, raise_on_error=False))
        if ra[0] != rb[0] or (ra[0] == "ok" and (not np.array_equal(ra[1][1], rb[1][1]) or np.nanmax(np.abs(np.where(ra[1][1] == 0, ra[1][0] - rb[1][0], 0.0)), initial=0.0) > 2e-6)):
            ok = False; why += " rmsd batch %r != %r" % (ra, rb)
        # the rotations of the two paths, frame by frame (the frames are still unfitted): what the comparison of the fitted coordinates below
        # is measured against.  Two correct fits of the same frame differ at atom i by at most |dR| |x_i - c| + |dt| (c: the group's centre,
        # about which both rotate): a difference in the ROTATION, which the group's own atoms barely see, is carried out to every other
        # atom of the system by its distance from the group.
        rots = []
        for f in range(nf):
            qa, qb = call(lambda: plans[0].rmsd(f, 1, return_rotation=True)), call(lambda: plans[1].rmsd(f, 1, return_rotation=True))
            rots.append((qa[1][2][0], qb[1][2][0]) if qa[0] == "ok" and qb[0] == "ok" and qa[1][1][0] == 0 and qb[1][1][0] == 0 else None)
        # the fit: one frame per call on S, the batch on B; the same statuses, rmsd and coordinates
        fa = [call(lambda: plans[0].rmsd_fit(f, 1)[0][0]) for f in range(nf)]
        fb = call(lambda: plans[1].rmsd_fit(0, nf, raise_on_error=False))
        for f in range(nf):
            if fb[0] != "ok": ok = False; why += " fit batch %r" % (fb,); break
            st_b = int(fb[1][1][f])
            if (fa[f][0] == "ok") != (st_b == 0): ok = False; why += " fit status[%d] %r / %d" % (f, fa[f], st_b)
            elif st_b == 0 and abs(float(fa[f][1]) - float(fb[1][0][f])) > 2e-6: ok = False; why += " fit rmsd[%d] %r / %r" % (f, fa[f][1], fb[1][0][f])
            pa, pb = S.get_positions(f), B.get_positions(f)
            # (one or two atoms -- or three in a line -- do not determine a rotation: H is rank-deficient and every path is free to turn the
            #  rest of the system about the group's axis; only the rmsd and the group's own atoms are comparable then)
            if ia.size < 4: pa, pb = pa[ia], pb[ia]
            # Bound.  The pair that came out 4.6e-5 nm apart under round 4's flat 3e-5 (seed 33: 6 252 atoms, a block of
            # 1 752, frame 2; tools/rot_debug.py on the dumped case) is a difference in the ROTATION, |dR|_F = 4.3e-5, and neither path is
            # wrong: the frame is an independent random blob (rmsd 0.98 nm), det H < 0, so the best PROPER rotation is U diag(1, 1, -1) V^T --
            # and that matrix is determined by H only to |dH| / (sigma_2 - sigma_3): here sigma = 14.99, 11.36, 11.21, a gap of 0.15 under
            # a covariance of size 22, i.e. 100 x the sensitivity of an ordinary fit (whose denominator is sigma_2 + sigma_3).  The single
            # wave forms H from exact fp64 products, the batched kernels from f32 chains: |dH| ~ 6e-6 -> |dR| ~ 4e-5; the oracle's own
            # answer moves by 1.4e-4 when the centre of the frame is displaced by 1e-6 nm.  So: rotations are compared against the
            # conditioning of THEIR problem, 1e-6 sigma_1 / (sigma_2 + sign(det H) sigma_3) + 3e-6, and fitted coordinates, atom by atom,
            # against 1.5e-5 (two f32 pipelines at |x| ~ 10 nm) + |dR|_F x the atom's distance from the group's centre.
            if not np.array_equal(np.isnan(pa), np.isnan(pb)):
                ok = False; why += " fitted coordinates[%d]: different atoms without position" % f
            elif st_b == 0 and fa[f][0] == "ok":
                d = np.abs(np.nan_to_num(pa - pb)).max(axis=1)
                if ia.size < 4 or rots[f] is None:
                    lim = np.full(d.shape, 3e-5)
                    dR = 0.0
                else:
                    dR = float(np.linalg.norm(rots[f][0].astype(np.float64) - rots[f][1].astype(np.float64)))
                    cen = np.nanmean(pb[ia] if pb.shape[0] == n else pb, axis=0)
                    lever = np.linalg.norm(np.nan_to_num(pb - cen), axis=1)
                    lim = 1.5e-5 + 1.05 * dR * lever
                    # conditioning of the rotation: H = sum (p - <p>)(q - <q>)^T over the group, reference against this frame's images
                    P = np.nan_to_num(ref.get_positions(0)[ia]).astype(np.float64); Q = np.nan_to_num(pb[ia] if pb.shape[0] == n else pb).astype(np.float64)
                    wts = np.nan_to_num(masses[ia], nan=1.0).astype(np.float64)[:, None]; wts_ref = ref_masses[ia].astype(np.float64)[:, None]
                    Hc = (P - (wts_ref * P).sum(0) / wts_ref.sum()).T @ (Q - (wts * Q).sum(0) / wts.sum())      # (unweighted, about the centres of mass: rmsd.rs:567-570)
                    sv = np.linalg.svd(Hc, compute_uv=False)
                    kappa = sv[0] / max(sv[1] + (1.0 if np.linalg.det(Hc) > 0 else -1.0) * sv[2], 1e-30)
                    if dR > 1e-6 * kappa + 3e-6:
                        ok = False; why += " rotations[%d] differ by %g with sigma1 / (sigma2 +- sigma3) = %g" % (f, dR, kappa)
                    worst_dr = max(worst_dr, dR)
                if (d > lim).any():
                    k = int(np.argmax(d - lim))
                    ok = False; why += " fitted coordinates[%d] differ by %g at atom %d (allowed %g, |dR| %g)" % (f, d[k], k, lim[k], dR)
                if d.max() > 3e-5 and ia.size >= 4 and rots[f] is not None:      # what the flat limit of round 4 would have flagged
                    k = int(np.argmax(d))
                    if os.environ.get("GR_FUZZ_DUMP") and not os.path.exists(os.environ["GR_FUZZ_DUMP"]):
                        np.savez(os.environ["GR_FUZZ_DUMP"], frames=np.stack(frames), masses=masses, ia=ia, box=box, f=f, scattered=(kind_a == "scattered"))
                    with O.acc64():
                        ro, want = O.calc_rmsd_and_fit(np.nan_to_num(frames[nf], nan=1.0), ref_masses, ia, box, frames[f], np.nan_to_num(masses, nan=1.0), ia, box)
                    print("note: n=%d group=%d frame %d: fitted coordinates %.3g apart at atom %d, %.2f nm from the group; |dR|_F %.3g, sigma1 / (sigma2 +- sigma3) %.3g; the group's own atoms %.3g apart; "
                          "against the oracle (fp64 sums): single wave %.3g, batched %.3g (group atoms %.3g / %.3g); rmsd %.7g: single wave %+.2g, batched %+.2g"
                          % (n, ia.size, f, d[k], k, lever[k], dR, kappa, float(d[ia].max()), float(np.nanmax(np.abs(pa - want))), float(np.nanmax(np.abs(pb - want))),
                             float(np.nanmax(np.abs(pa[ia] - want[ia]))), float(np.nanmax(np.abs(pb[ia] - want[ia]))), ro, float(fa[f][1]) - ro, float(fb[1][0][f]) - ro), flush=True)
                worst_xyz = max(worst_xyz, float(d.max()))
        for p in plans: p.close()
    # the oracle on frame nf (never poisoned, never fitted): COM of group b
    if not np.isnan(masses[ib]).any():
        with O.acc64():
            want = O.get_center(frames[nf], ib, box, mass=masses)
        got = call(lambda: S.group_get_com("b", slot=nf))
        if got[0] != "ok" or np.abs(got[1] - want).max() > 1e-5: ok = False; why += " oracle COM %r != %r" % (got, want)
    small_total += S.stat("small_calls")
    if S.stat("small_sync_fallbacks"): ok = False; why += " sync fallbacks"
    if B.stat("small_calls"): ok = False; why += " the batched twin took the single-wave path"
    cases += 1
    bad += 0 if ok else 1
    if cases <= 30 or not ok:
        print("%s n=%d a=%s(%d) b=%s(%d) cell=%s frames=%d %s%s%s%s" % ("ok " if ok else "BAD", n, kind_a, ia.size, kind_b, ib.size, "/".join("%g" % x for x in angles), nf,
                                                                      "wide " if wide else "", "poisoned " if poison else "", "own-weights " if own_w else "", why), flush=True)
    for x in (S, B, ref): x.close()
print("largest |dR|_F between the two paths %.3g, fitted coordinates at most %.3g nm apart" % (worst_dr, worst_xyz))
print("%d cases, %d mismatches, %d calls answered by the single-wave kernels; %d ill-conditioned cases (a group spread over the whole cell) not compared" % (cases, bad, small_total, ill))
sys.exit(1 if bad else 0)
