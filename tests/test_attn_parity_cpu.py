"""The float64 attention parity checker (tests/attn_parity.py) tested on the CPU:

  - a CORRECT kernel - the float32 / bf16 emulation of attn_parity.emulate - passes both tiers for every case and regime of the GPU
    list (which also proves that the inputs keep the kernels' own arithmetic inside the bounds);
  - twelve seeded defects, each planted into a copy of the float64 reference on ONE tile, head, row or batch element, all fail, in
    every case and regime they apply to;
  - the same defects under the metric of tests/test_kernels_gpu.py (max |got - ref| / max |ref| over the tensor below 2.5e-2 for
    bf16, 1e-4 for f32) are printed: a record of what that metric misses, not an assertion;
  - every family meets every input regime, and the dispatch dry run (pa_attn_plan, no device) sends every case to the kernels it names,
    under its own switch bundle (children: the switches are read once per process); together the cases name every kernel of
    tests/golden/attn_plan.json.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import attn_parity as ap
import dropout_masks as dm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ap.cases()
IDS = [c["name"] for c in ALL]
MISSED_BY_OLD_METRIC = {}                                            # defect -> [applied, passed the old metric]


# ------------------------------------------------------------------------------------------------ where the defects go
def pick_element(c, t):
    """The batch element with the most allowed (query, key) pairs."""
    best, best_n = None, 0
    for b, (_, nq, _, nk) in enumerate(t.el):
        n = int(t.allowed(b).sum()) if nq and nk else 0
        if n > best_n:
            best, best_n = b, n
    return best


def pick_short_element(c, t, at_least=16):
    """The batch element with the fewest keys (at least `at_least` of them and of query rows): a defect on ONE tile is a large share of
    such an element, while its share of a long one (20 % of one ninth of the mass) is inside the bound of a correct bf16 kernel."""
    ok = [(e[3], b) for b, e in enumerate(t.el) if e[1] >= at_least and e[3] >= at_least and t.allowed(b).any()]
    return min(ok)[1] if ok else pick_element(c, t)


def on_element(c, t, b0, hook):
    """The float64 reference with `hook` applied to batch element b0 (everything else as the good reference)."""
    good_only = ap.reference(c, t, scales=False, only={b0})
    bad_only = ap.reference(c, t, element_hook=lambda b, *a: hook(*a) if b == b0 else a, scales=False, only={b0})
    return good_only, bad_only


def graft(good, good_only, bad_only):
    return {k_: good[k_] + (bad_only[k_] - good_only[k_]) for k_ in ap.OUTPUTS}


def _extend(k, v, allowed, D, rows_k, rows_v, c, t, b0):
    """Lengthen the keys of an element by rows_k / rows_v [H, n, dh]: allowed (causal still holds), with their own dropout decisions."""
    H, nq, nk = allowed.shape
    n = rows_k.shape[1]
    extra = np.ones((H, nq, n), dtype=bool)
    if c["causal"]:
        extra &= (np.arange(nk, nk + n)[None, :] <= np.arange(nq)[:, None])[None]
    if D is not None:
        rows = (b0 * H + np.arange(H)[:, None]) * c["Lq"] + np.arange(nq)[None, :]
        D = dm.attn_keep(ap.DROP_SEED, rows, nk + n, c["drop"]) * dm.attn_scale(c["drop"])
    return np.concatenate([k, rows_k], 1), np.concatenate([v, rows_v], 1), np.concatenate([allowed, extra], 2), D


def heavy_tile(c, t, b0, h0, rows):
    """First key of the 64-key tile that holds the most probability mass of query rows [0, rows) of head h0: a defect planted on a tile
    whose probabilities vanish (the early tiles of a rising ramp) is no defect of the function."""
    s2, _, _ = _unnormalised(c, t, b0)
    s = s2[h0, :rows]
    with np.errstate(invalid="ignore"):
        e = np.where(np.isfinite(s), np.exp2(s - np.where(np.isfinite(s.max(-1)), s.max(-1), 0.0)[:, None]), 0.0)
    p = e / np.maximum(e.sum(-1), 1e-300)[:, None]
    mass = np.add.reduceat(p.sum(0), np.arange(0, s.shape[1], 64))
    return 64 * int(np.argmax(mass))


# ------------------------------------------------------------------------------------------------ the seeded defects
# each: (c, t, good) -> the defective outputs (float64, before the store), or None where the defect does not apply to the case
def d_key_tile_skipped(c, t, good):
    b0 = pick_element(c, t)
    h0 = c["H"] - 1

    k_ = heavy_tile(c, t, b0, h0, 128)

    def hook(q, k, v, do, allowed, D):
        allowed[h0, :128, k_:k_ + 64] = False
        return q, k, v, do, allowed, D
    return graft(good, *on_element(c, t, b0, hook))


def d_ragged_tail_valid(c, t, good):
    """The keys past the end of the LAST element's ragged tile counted as valid: they are the rows that follow in the buffer (2^60)."""
    b0 = max(b for b, e in enumerate(t.el) if e[1] and e[3])
    nk = t.el[b0][3]
    if nk % 64 == 0 or t.el[b0][2] + nk != t.Rk or (c["causal"] and t.el[b0][1] <= nk):
        return None                                                 # (causal with no query past the last key: j <= i masks the tail anyway)
    n = min(64 - nk % 64, 4)

    def hook(q, k, v, do, allowed, D):
        pad = np.full((k.shape[0], n, k.shape[2]), ap.POISON)
        k, v, allowed, D = _extend(k, v, allowed, D, pad, pad, c, t, b0)
        return q, k, v, do, allowed, D
    with np.errstate(all="ignore"):
        return graft(good, *on_element(c, t, b0, hook))


def d_causal_diagonal_excluded(c, t, good):
    if not c["causal"]:
        return None
    b0 = pick_element(c, t)

    def hook(q, k, v, do, allowed, D):
        n = min(64, allowed.shape[1], allowed.shape[2])
        allowed[-1, :n, :n] &= np.arange(n)[None, :] < np.arange(n)[:, None]
        return q, k, v, do, allowed, D
    return graft(good, *on_element(c, t, b0, hook))


def d_mask_hole_ignored(c, t, good):
    if t.kpm is None:
        return None
    b0 = pick_element(c, t)
    holes = np.nonzero(t.kpm[b0, :t.el[b0][3]])[0]
    if not len(holes):
        return None

    def hook(q, k, v, do, allowed, D):
        allowed[0, :, holes[0]] = True if not c["causal"] else (holes[0] <= np.arange(allowed.shape[1]))
        return q, k, v, do, allowed, D
    return graft(good, *on_element(c, t, b0, hook))


def d_dropout_scale_missing(c, t, good):
    if not c["drop"]:
        return None
    b0 = pick_short_element(c, t)

    k_ = heavy_tile(c, t, b0, c["H"] - 1, 128)

    def hook(q, k, v, do, allowed, D):
        D = D.copy()
        D[-1, :128, k_:k_ + 64] /= dm.attn_scale(c["drop"])
        return q, k, v, do, allowed, D
    return graft(good, *on_element(c, t, b0, hook))


def d_dropout_transposed(c, t, good):
    if not c["drop"]:
        return None
    b0 = pick_short_element(c, t)

    k_ = heavy_tile(c, t, b0, c["H"] - 1, 64)

    def hook(q, k, v, do, allowed, D):
        n = min(64, D.shape[1], D.shape[2] - k_)
        D = D.copy()
        D[-1, :n, k_:k_ + n] = D[-1, :n, k_:k_ + n].T.copy()
        return q, k, v, do, allowed, D
    return graft(good, *on_element(c, t, b0, hook))


def _unnormalised(c, t, b0):
    """Log2-domain scores (masked: -inf), dropout weights and V of element b0 in float64: [H, Lq, Lk], [H, Lq, Lk], [H, Lk, dh]."""
    q0, nq, k0, nk = t.el[b0]
    q, k, v = ap._hfirst(t.q, q0, nq), ap._hfirst(t.k, k0, nk), ap._hfirst(t.v, k0, nk)
    allowed = np.broadcast_to(t.allowed(b0), (c["H"], nq, nk))
    with np.errstate(invalid="ignore", over="ignore"):
        s2 = np.where(allowed, t.scale * ap.LOG2E * np.einsum("hic,hjc->hij", q, np.where(np.abs(k) >= ap.MASKED_KV, 0.0, k)), -np.inf)
    keep = t.keep(b0)
    D = np.ones_like(s2) if keep is None else keep * dm.attn_scale(c["drop"])
    return s2, D, np.where(np.abs(v) >= ap.MASKED_KV, 0.0, v)


def d_accumulator_not_rescaled(c, t, good):
    """Online softmax over 64-key tiles, deferred rescale decided per 16-row wave (threshold 2^8): when the reference point moves, l is
    rescaled and the accumulated O is not - old terms keep their weight.  Applies where the regime moves the reference after the first
    tile: `steps` and `late_spike`."""
    if c["regime"] not in ("steps", "late_spike"):
        return None
    b0 = pick_element(c, t)
    q0, nq, k0, nk = t.el[b0]
    if nk <= 64:
        return None
    s2, D, v = _unnormalised(c, t, b0)
    H = c["H"]
    m = np.full((H, nq), -np.inf)
    l = np.zeros((H, nq))
    acc = np.zeros((H, nq, c["dh"]))
    wave = np.arange(nq) // 16
    with np.errstate(invalid="ignore", over="ignore"):
        for k_ in range(0, nk, 64):
            st = s2[:, :, k_:k_ + 64]
            mx = st.max(-1)
            grew = mx > np.where(np.isfinite(m), m + 8.0, -np.inf)
            for w in range(wave.max() + 1):                         # the test is wave-wide
                rows = wave == w
                move = grew[:, rows].any(-1)                        # [H]
                m_new = np.where(move[:, None], np.maximum(m[:, rows], mx[:, rows]), m[:, rows])
                alpha = np.where(np.isfinite(m[:, rows]) & np.isfinite(m_new), np.exp2(m[:, rows] - m_new), 1.0)
                l[:, rows] *= alpha                                 # (and acc is NOT: the defect)
                m[:, rows] = m_new
            ms = np.where(np.isfinite(m), m, 0.0)
            e = np.where(np.isfinite(st), np.exp2(st - ms[..., None]), 0.0)
            l += e.sum(-1)
            acc += np.einsum("hij,hjc->hic", e * D[:, :, k_:k_ + 64], v[:, k_:k_ + 64])
        o = acc / np.where(l > 0, l, 1.0)[..., None]
    bad = {k_: good[k_].copy() for k_ in ap.OUTPUTS}
    bad["o"][q0:q0 + nq] = o.transpose(1, 0, 2)
    return bad


def d_split_merge_unweighted(c, t, good):
    """The in-block key split (v4 forward, KS = 2): the two key halves merged with a0 = a1 = 1 instead of 2^(m_h - m)."""
    if c["fwd"] != "v4ks":
        return None
    b0 = pick_element(c, t)
    q0, nq, k0, nk = t.el[b0]
    ksteps = (nk + 63) // 64
    if ksteps < 4:
        return None
    cut = (ksteps + 1) // 2 * 64
    s2, D, v = _unnormalised(c, t, b0)
    acc, l = 0.0, 0.0
    for lo, hi in ((0, cut), (cut, nk)):
        sh = s2[:, :, lo:hi]
        e = np.exp2(sh - sh.max(-1, keepdims=True))
        l = l + e.sum(-1)
        acc = acc + np.einsum("hij,hjc->hic", e * D[:, :, lo:hi], v[:, lo:hi])
    bad = {k_: good[k_].copy() for k_ in ap.OUTPUTS}
    bad["o"][q0:q0 + nq] = (acc / l[..., None]).transpose(1, 0, 2)
    return bad


def d_lse_misses_a_tile(c, t, good):
    """lse of one row without the mass of one 64-key tile (the row's heaviest)."""
    b0 = pick_element(c, t)
    q0, nq, k0, nk = t.el[b0]
    if nk <= 64:
        return None
    s2, _, _ = _unnormalised(c, t, b0)
    row = s2[0, nq - 1]
    e = np.exp2(row - row.max())
    mass = np.add.reduceat(e, np.arange(0, nk, 64))
    if mass.max() >= e.sum() * (1 - 1e-9):
        return None                                                 # (one tile holds everything: nothing is left to take the log of)
    bad = {k_: good[k_].copy() for k_ in ap.OUTPUTS}
    bad["lse"][b0, 0, nq - 1] = (row.max() + np.log2(e.sum() - mass.max())) * ap.LN2
    return bad


def d_dk_without_scale(c, t, good):
    bad = {k_: good[k_].copy() for k_ in ap.OUTPUTS}
    bad["dk"][:, c["H"] - 1] /= t.scale
    return bad


def d_cu_k_off_by_one(c, t, good):
    """Element b reads one key row of the element that follows it in the packed K / V."""
    if c["layout"] == "dense":
        return None
    cand = [(e[3], b) for b, e in enumerate(t.el) if e[1] and e[3] and e[2] + e[3] < t.Rk]
    if not cand:
        return None
    b0 = min(cand)[1]                                               # (the shortest element: one more key is a large share of it)
    k_end = t.el[b0][2] + t.el[b0][3]

    def hook(q, k, v, do, allowed, D):
        k, v, allowed, D = _extend(k, v, allowed, D, ap._hfirst(t.k, k_end, 1), ap._hfirst(t.v, k_end, 1), c, t, b0)
        return q, k, v, do, allowed, D
    return graft(good, *on_element(c, t, b0, hook))


def d_keyless_row_left_at_the_pattern(c, t, good):
    for b, (q0, nq, _, nk) in enumerate(t.el):
        none = ~t.allowed(b).any(-1) if nk else np.ones(nq, dtype=bool)
        if nq and none.any():
            bad = {k_: good[k_].copy() for k_ in ap.OUTPUTS}
            bad["o"][q0 + int(np.nonzero(none)[0][0]), 0] = ap.PATTERN
            return bad
    return None


DEFECTS = [d_key_tile_skipped, d_ragged_tail_valid, d_causal_diagonal_excluded, d_mask_hole_ignored, d_dropout_scale_missing,
           d_dropout_transposed, d_accumulator_not_rescaled, d_split_merge_unweighted, d_lse_misses_a_tile, d_dk_without_scale,
           d_cu_k_off_by_one, d_keyless_row_left_at_the_pattern]


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_the_emulation_passes_and_every_seeded_defect_fails(c):
    t = ap.Tensors(c)
    ref = ap.reference(c, t)
    emu = ap.stored(c, ap.emulate(c, t))
    rs = ap.check_all(c, emu, ref, emu)                              # a correct kernel: tier 1 (tier 2 against itself holds trivially)
    for what, (r, _) in rs.items():
        assert 0 <= r < 2.0, (what, r)
    good = {k_: ref[k_] for k_ in ap.OUTPUTS}
    ap.check_all(c, ap.stored(c, good), ref, emu)                    # the reference itself, stored: inside both tiers
    for defect in DEFECTS:
        bad = defect(c, t, good)
        if bad is None:
            continue
        got = ap.stored(c, bad)
        try:
            ap.check_all(c, got, ref, emu)
        except AssertionError as e:
            assert "tier 1" in str(e) or "tier 2" in str(e), e
        else:
            pytest.fail(f"{c['name']}: {defect.__name__} goes unseen")
        tally = MISSED_BY_OLD_METRIC.setdefault(defect.__name__, [0, 0])
        tally[0] += 1
        tally[1] += int(ap.old_metric_passes(c, got, ref))


def test_old_metric_table(capsys):
    """Which of the seeded defects max |got - ref| / max |ref| < tol over the tensor misses (printed, not asserted)."""
    with capsys.disabled():
        print("\n  seeded defect                          cases   pass the tensor-wide metric of tests/test_kernels_gpu.py")
        for d in DEFECTS:
            n, missed = MISSED_BY_OLD_METRIC.get(d.__name__, (0, 0))
            print(f"  {d.__name__[2:]:38s} {n:5d}   {missed:5d}")
    if MISSED_BY_OLD_METRIC:                                         # (empty when this test is selected alone)
        assert all(MISSED_BY_OLD_METRIC.get(d.__name__, (0, 0))[0] > 0 for d in DEFECTS), "a seeded defect applies to no case"


def test_every_family_meets_every_regime_and_dropout():
    seen = {(f, c["regime"]) for c in ALL for f in (c["fam"], c["bfam"])}
    missing = [(f, r) for f in ap.FAMILIES for r in ap.REGIMES if (f, r) not in seen]
    assert not missing, missing
    for f in ap.FAMILIES:
        assert any(c["drop"] for c in ALL if f in (c["fam"], c["bfam"])), f


def test_the_cases_name_every_kernel():
    golden = set(json.load(open(os.path.join(REPO, "tests", "golden", "attn_plan.json")))["names"])
    named = set()
    for c in ALL:
        f, b = ap.kernel_names(c)
        named.update(f + b)
    assert named == golden, (sorted(golden - named), sorted(named - golden))


def _assert_plans(bundle):
    from plankassembly_amd import _lib as L
    off = []
    for c in ALL:
        if c["bundle"] == bundle:
            got, want = ap.planned_names(L, c), list(ap.kernel_names(c))
            if got != want:
                off.append((c["name"], got, want))
    assert not off, off


@pytest.mark.parametrize("bundle", list(ap.BUNDLES))
def test_the_dry_run_sends_every_case_to_the_kernels_it_names(bundle):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PA_ATTN_", "PA_X3_"))}
    env.update(ap.BUNDLES[bundle], PYTHONPATH=os.pathsep.join([REPO, os.path.join(REPO, "tests"), env.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plan", bundle], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "plans ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


if __name__ == "__main__":
    assert sys.argv[1] == "--plan"
    _assert_plans(sys.argv[2])
    print("plans ok")
