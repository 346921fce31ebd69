"""The training step's host-side plan ("how big is the workspace, which split-K and which slab does every weight gradient of a
backward segment get") pinned without a GPU, through pa_train_plan - the dry run of pa_model_train_ws_bytes and of the plan
pa_model_train_bwd makes before each segment (include/plank_hip.h).  tests/golden/train_plan.json holds, for every case, the status
or: the workspace bytes of the commit BEFORE the plan function existed, and per segment kind (heads, decoder layer, encoder layer)
every member's split-K and slab offset in floats (-1: no slab).

How the golden file was made: from that earlier commit, not from the code under test.  In a scratch copy of its csrc/runtime.hip
one throwaway export was appended that created a model, called pa_train_layout(m, NULL, B, S, T), set defer_ok and the row counts,
called that commit's own Ctx::linear_dw once per member of a segment kind (dummy non-null operands, db = NULL: with the default
switches every member is queued and nothing is launched), then called its plan_group and returned each queued member's M, N, K,
splitk and ws offset, next to that commit's pa_model_train_ws_bytes.  That library, built with the project's flags, ran record() of
this file with the export as `plan_case`.  The status of a case is what that commit's pa_model_create, then its
pa_model_train_ws_bytes answered; a packed row count outside 1..B*S is the PA_EINVAL its pa_model_train_fwd answered for such a
batch.  The recording also checked that the queued (M, N, K) are members() below.  The scratch export is not committed.

The workspace shrank with the side stream's second buffer set: the golden bytes minus removed_bytes() (every removed take written
out, each rounded up to the arena's 256 bytes) must be the bytes reported now.  Every take starts 256-aligned and the arena's end is
not rounded; the last removed take (the second slab area) has the size of the take that is last now, so the difference is exact.

Every f32 case is planned twice: exact, and under the bf16x3 mode (pa_gemm_split_config(1, ..) only stores its arguments).
"""
import ctypes as C
import itertools
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "train_plan.json")
sys.path.insert(0, REPO)

PA_F32, PA_BF16 = 0, 1
CODE_OF_STATUS = {-1: "I", -2: "A", -3: "S"}
VOCAB, LDV = 514, 576                                          # (logit rows are padded to a whole K tile of 64)
KINDS = ("heads", "decoder layer", "encoder layer")

DTYPES = [PA_BF16, PA_F32]
# (d_model, heads): head dims 64 / 32 / 64 / 64 / 64
WIDTHS = [(64, 1), (256, 8), (512, 8), (768, 12), (1024, 16)]
FFS = [256, 1024, 4096]
NDECS = [0, 1, 6]
BS, SS, TS = [1, 16, 256], [1, 100, 1199], [1, 12, 1024]
N_SAMPLED = 60

# (dtype, d_model, n_head, d_ff, n_enc, n_dec, B, S, T, n_valid); n_valid 0: unpacked rows
# the benchmark's model (d_model 512, 8 heads, d_ff 1024, 6 + 6 layers) and its batch of 16 full-length drawings
HEADLINE_BF16 = (PA_BF16, 512, 8, 1024, 6, 6, 16, 1199, 128, 7940)
HEADLINE_F32 = (PA_F32, 512, 8, 1024, 6, 6, 16, 1199, 128, 7940)
INVALID = [
    (PA_BF16, 512, 8, 1024, 6, 6, 0, 1199, 128, 0), (PA_BF16, 512, 8, 1024, 6, 6, 16, -1, 128, 0),     # B, S
    (PA_F32, 512, 8, 1024, 6, 6, 16, 1199, 0, 0),                                                       # T
    (PA_BF16, 512, 8, 1024, 6, 6, 16, 1199, 128, -5), (PA_F32, 512, 8, 1024, 6, 6, 16, 1199, 128, 16 * 1199 + 1),   # n_valid
    (PA_BF16, 512, 0, 2048, 6, 6, 16, 1199, 128, 0), (PA_BF16, 512, 3, 2048, 6, 6, 16, 1199, 128, 0),   # no heads; heads that do not divide
    (PA_BF16, 0, 8, 2048, 6, 6, 16, 1199, 128, 0),                                                      # d_model
    (PA_BF16, 512, 4, 2048, 6, 6, 16, 1199, 128, 0), (PA_F32, 768, 16, 2048, 6, 6, 16, 1199, 128, 0),   # head dims 128 and 48
    (PA_BF16, 512, 8, 2044, 6, 6, 16, 1199, 128, 0),                                                    # d_ff no multiple of 8
    (7, 512, 8, 1024, 6, 6, 16, 1199, 128, 0),                                                          # dtype
]


def cases():
    """The case list, in a fixed order:
      - the headline model in both dtypes at every (B, S, T): unpacked, and packed to 1, 7940 and B*S rows where B*S allows: 180,
      - every width x d_ff x n_dec in both dtypes at the headline batch (d_model 1024 x d_ff 4096 has the 256-tile members): 90,
      - an invalid argument of each kind: 12,
      - N_SAMPLED shapes drawn from the product by a fixed linear congruential sequence (invalid combinations stay in)."""
    out = []
    for dt, B, S, T in itertools.product(DTYPES, BS, SS, TS):
        out += [(dt, 512, 8, 1024, 6, 6, B, S, T, nv) for nv in (0, 1, 7940, B * S) if nv <= B * S and (nv != 1 or B * S > 1)]
    out += [(dt, d, H, ff, 6, nd, 16, 1199, 128, 7940) for dt, (d, H), ff, nd in itertools.product(DTYPES, WIDTHS, FFS, NDECS)]
    out += INVALID
    dims = [DTYPES, WIDTHS + [(512, 16), (768, 16)], FFS + [520, 2048], [0, 1, 6], NDECS, BS + [0, 31], SS + [0, 640], TS + [0, 24],
            [0, 0, 1, 7940, -1]]
    x = 12345
    for _ in range(N_SAMPLED):
        pick = []
        for d in dims:
            x = (x * 1103515245 + 12345) % (1 << 31)
            pick.append(d[(x >> 8) % len(d)])
        out.append((pick[0], *pick[1], *pick[2:]))
    return out


def planned(cs=None):
    """(case, x3) in the order of the golden rows: every f32 case is followed by itself under the bf16x3 mode."""
    return [(c, x3) for c in (cs or cases()) for x3 in ((0, 1) if c[0] == PA_F32 else (0,))]


def model_cfg(case):
    """The pa_model_cfg of a case (what the plan does not read is the shipped configuration's)."""
    from plankassembly_amd.models import _ModelCfg
    dt, d, H, ff, ne, nd = case[:6]
    c = _ModelCfg()
    c.d_model, c.n_head, c.d_ff, c.n_enc, c.n_dec, c.vocab, c.out_dof = d, H, ff, ne, nd, VOCAB, 6
    c.eps_layer, c.eps_final, c.has_enc_norm, c.dropout, c.pad, c.end, c.dtype, c.activation = 1.0, 1e-5, 1, 0.0, 513, 512, dt, 1
    return c


def members(case):
    """Per segment kind the weight gradients in the order the backward queues them: (rows, cols) of dW and the contraction length."""
    _, d, _, ff, _, _, B, S, T, nv = case
    BT, NE = B * T, (nv if nv > 0 else B * S)
    return [[(VOCAB, d, BT), (d, d, BT)],
            [(d, ff, BT), (ff, d, BT), (d, d, BT), (d, d, BT), (2 * d, d, NE), (d, d, BT), (3 * d, d, BT)],
            [(d, ff, NE), (ff, d, NE), (d, d, NE), (3 * d, d, NE)]]


def splitws_floats(case):
    _, d, _, ff = case[:4]
    return 16 * max(8 * d * d + 2 * d * ff + LDV * d, 3 * d * d, d * ff)


def removed_bytes(case, lib):
    """The takes of the second buffer set (the side stream's), as pa_train_layout made them before this plan existed."""
    dt, d, _, ff, _, _, B, S, T, _ = case
    e = 2 if dt == PA_BF16 else 4
    BS_, R = B * S, max(B * S, B * T)
    ln = int(lib.pa_layernorm_ws_floats(R, d)) * 4
    takes = [R * d * e] * 6                                     # three per-site dz buffers and their dropped twins
    takes += [R * d * e, R * ff * e, R * 3 * d * e, BS_ * 2 * d * e]      # gE, gF, gQ3, gKV
    takes += [ln] * 3                                           # queued LayerNorm-backward partials
    takes += [splitws_floats(case) * 4]                         # split-K slab area
    return sum(-(-t // 256) * 256 for t in takes)


class X3:
    """The bf16x3 mode around a block: without a GPU, over an address nothing is ever written to."""

    def __init__(self, lib, on):
        self.lib, self.on = lib, on

    def __enter__(self):
        if self.on:
            assert self.lib.pa_gemm_split_config(1, C.c_void_p(1 << 20), C.c_int64(1 << 20)) == 0

    def __exit__(self, *exc):
        assert self.lib.pa_gemm_split_config(0, None, 0) == 0


def record(lib, plan_case=None):
    """One row per planned(): a status letter, or [ws_bytes, [[splitk, slab], ...] per kind].  plan_case(cfg, case) -> (status, ws_bytes,
    [[(rows, cols, k, splitk, slab), ...] x 3]): how a case is planned (the recording of the golden file put the export here)."""
    from plankassembly_amd import _lib as L

    def dry_run(cfg, case):
        info = L.TrainPlanInfo()
        rc = lib.pa_train_plan(C.byref(cfg), *case[6:], C.byref(info))
        if rc:
            return rc, 0, None
        assert info.n_segments == case[4] + case[5] + 4 and info.splitws_floats == splitws_floats(case)
        return 0, info.ws_bytes, [[(m.rows, m.cols, m.k, m.splitk, m.slab) for m in info.member[k][:info.n_members[k]]] for k in range(3)]

    rows = []
    for case, x3 in planned():
        with X3(lib, x3):
            rc, ws, kinds = (plan_case or dry_run)(model_cfg(case), case)
        if rc:
            rows.append(CODE_OF_STATUS[rc])
            continue
        assert [[m[:3] for m in k] for k in kinds] == members(case), (case, kinds)
        rows.append([ws, [[list(m[3:]) for m in k] for k in kinds]])
    return rows


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(REPO, "plankassembly_amd", "libplank_hip.so")):
        from plankassembly_amd.build import build
        build()
    from plankassembly_amd import _lib as L
    return L.lib()


@pytest.fixture(scope="module")
def rows(lib):
    return record(lib)


def test_case_list_matches_the_golden_file():
    gold = json.load(open(GOLDEN))
    cs = cases()
    assert 280 <= len(cs) <= 360 and gold["cases"] == len(cs) and len(gold["rows"]) == len(planned(cs))
    assert os.path.getsize(GOLDEN) < 256 * 1024
    ok = [r for r in gold["rows"] if not isinstance(r, str)]
    assert len(ok) > 400 and {r for r in gold["rows"] if isinstance(r, str)} == {"I", "S"}
    # the golden file exercises the rule: members that stay whole, splits all the way up to the cap of 16, and 256-tile members
    splits = {m[0] for r in ok for k in r[1] for m in k}
    assert {1, 2, 16} <= splits <= set(range(1, 17)) and len(splits) >= 12, splits
    assert any(c[1] == 1024 and c[3] == 4096 for (c, _), r in zip(planned(cs), gold["rows"]) if not isinstance(r, str))


def test_every_split_and_slab_is_the_recorded_one(rows):
    want = json.load(open(GOLDEN))["rows"]
    pl = planned()
    assert len(rows) == len(pl) == len(want)
    wrong = [(c, x3, got, w) for (c, x3), got, w in zip(pl, rows, want)
             if (got != w if isinstance(got, str) or isinstance(w, str) else got[1] != w[1])]
    assert not wrong, f"{len(wrong)} of {len(pl)} plans differ from the recorded rule, first: {wrong[:3]}"


def test_workspace_is_the_recorded_one_minus_the_second_buffer_set(rows, lib):
    want = json.load(open(GOLDEN))["rows"]
    n = 0
    for (case, x3), got, w in zip(planned(), rows, want):
        if isinstance(w, str):
            continue
        n += 1
        assert got[0] == w[0] - removed_bytes(case, lib), (case, x3, got[0], w[0], removed_bytes(case, lib))
    assert n > 400


def test_plans_are_consistent_independent_of_the_golden_file(rows):
    for (case, x3), row in zip(planned(), rows):
        if isinstance(row, str):
            continue
        bf = case[0] == PA_BF16 or x3
        for kind, mem in zip(row[1], members(case)):
            off, deferred = 0, 0
            for (sk, slab), (r, c, k) in zip(kind, mem):
                tiles = -(-r // 128) * -(-c // 128)
                nkt = -(-(3 * k if x3 else k) // (64 if bf else 16))
                assert 1 <= sk <= max(1, min(16, nkt // 4)) and (tiles < 256 or sk == 1), (case, x3, kind)
                assert (slab >= 0) == (sk > 1), (case, x3, kind)
                if sk > 1:
                    assert slab == off and slab % 4 == 0 and slab + sk * r * c <= splitws_floats(case), (case, x3, kind)
                    off = slab + -(-sk * r * c // 4) * 4
                    deferred += 1
            assert deferred <= 16


def test_anchors(rows):
    """Readable anchors at the headline batch (16 drawings packed to 7940 rows, 128 output tokens)."""
    by = dict(zip(planned(), rows))
    heads, dec, enc = by[(HEADLINE_BF16, 0)][1]
    # bf16 heads: 20 + 16 tiles over 32 K tiles (2048 rows): seven slices each fill the round of 256 (252), slabs back to back
    assert heads == [[7, 0], [7, 7 * VOCAB * 512]]
    # bf16 decoder layer: 192 tiles; only the cross-attention K|V gradient (125 K tiles of encoder rows, 32 tiles) is longer than the
    # others (32 K tiles): two more slices of it fill the round
    assert dec == [[1, -1]] * 4 + [[3, 0]] + [[1, -1]] * 2
    # bf16 encoder layer: 128 tiles over 125 K tiles each: every member split in two fills the round; slabs back to back
    assert enc == [[2, 0], [2, 2 * 512 * 1024], [2, 4 * 512 * 1024], [2, 4 * 512 * 1024 + 2 * 512 * 512]]
    # bf16x3 plans like bf16 over 3 K: the same splits at this shape; the workspace is the f32 one
    assert by[(HEADLINE_F32, 1)][1] == by[(HEADLINE_BF16, 0)][1] and by[(HEADLINE_F32, 0)][0] == by[(HEADLINE_F32, 1)][0]
    # exact f32 plans every member for the whole chip: 512 / tiles, at most 16
    assert [m[0] for m in by[(HEADLINE_F32, 0)][1][2]] == [16, 16, 16, 10]


def test_null_arguments(lib):
    from plankassembly_amd import _lib as L
    info = L.TrainPlanInfo()
    cfg = model_cfg(HEADLINE_BF16)
    assert lib.pa_train_plan(None, 4, 40, 12, 0, C.byref(info)) == -1
    assert lib.pa_train_plan(C.byref(cfg), 4, 40, 12, 0, None) == -1
