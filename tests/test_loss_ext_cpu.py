"""CPU checks of the extended mixture NLL: the float64 restatement of tests/loss_ext_reference.py against torch
autograd, the float32 restatement under the checker on the whole case table, the checker on seeded defects, the mirror of pa_loss_ext,
and the argument checks of the Python surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import loss_ext_reference as R
import rowops_parity as rp
from plankassembly_amd import _lib as L
from plankassembly_amd.trainer import Trainer
from test_trainer_surface import small_hparams

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = rp.nll_cases()


# ------------------------------------------------------------------------------------------------ 1: float64 restatement = autograd
def _small_case(B, T, V):
    """nll_inputs of a (B, T, V) case, with the last drawing's labels redrawn so that it ends in a PAD tail instead of being PAD throughout
    (a zero or negative weight then meets real rows)."""
    c = dict(kernel="nll", name=f"loss_ext_B{B}_T{T}_V{V}", B=B, T=T, V=V, ldv=V, scale=1, allpad=0)
    t = rp.nll_inputs(c)
    g = torch.Generator().manual_seed(rp.seed_of(c["name"], 5))
    lab = t["label"].view(B, T)
    i = torch.arange(T)
    fresh = torch.where(torch.rand(T, generator=g) < 0.5, torch.randint(0, V, (T,), generator=g), V + (torch.rand(T, generator=g) * (i + 1)).long().clamp(max=T - 1))
    lab[B - 1] = fresh
    lab[B - 1, T - 3:] = t["pad"]
    return c, t


def _dists64(c, t, x, z, s):
    """create_dist_train of oracle/plank_oracle.py on given logits (the fill is the float32 1e-6 the kernels hold), torch float64."""
    B, T, V = c["B"], c["T"], c["V"]
    tri = torch.triu(torch.ones(T, T)) == 1
    zz = z.view(B, T, T).masked_fill(tri[None], rp.C6)
    prob = torch.sigmoid(s).view(B, T, 1)
    vd = torch.log_softmax(x.view(B, T, V), -1) + torch.log(torch.clamp(1 - prob, min=rp.C6))
    pd = torch.log_softmax(zz, -1) + torch.log(torch.clamp(prob, min=rp.C6))
    return torch.cat((vd, pd), -1)


@pytest.mark.parametrize("shape", [(2, 9, 7), (2, 36, 514)])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("wsel", ["none", "neg_zero", "zero_neg"])
def test_float64_restatement_equals_autograd(shape, eps, wsel):
    c, t = _small_case(*shape)
    B, T, V = shape
    w = {"none": None, "neg_zero": torch.tensor([-0.5, 0.0]), "zero_neg": torch.tensor([0.0, -0.5])}[wsel]
    x, z, s = (t[k].double().clone().requires_grad_(True) for k in ("vocab", "ptr", "sw"))
    loss, mean, token = R.loss_from_dists(_dists64(c, t, x, z, s), t["label"].view(B, T), t["pad"], eps, w)
    up, gscale = 0.75, 0.25
    (loss * up * gscale).backward()
    ref = R.ext_fwd_ref(c, t, eps, w)
    assert ref["count"] == int((t["label"] != t["pad"]).sum()) and ref["count"] > T
    assert abs(ref["loss"][0] - loss.item()) <= 1e-12 and abs(ref["mean"][0] - mean.item()) <= 1e-12
    assert np.abs(ref["token"][0] - token.detach().numpy().reshape(-1)).max() <= 1e-12
    # the reference's gradients from ITS OWN float64 row_lse and count (what the kernels read back as float32 is an input of the GPU test)
    lse = torch.from_numpy(np.stack([ref["R"]["lse_v"], ref["R"]["lse_p"]], 1))
    b = R.ext_bwd_ref(c, t, eps, w, lse, np.float64(ref["count"]), np.float64(up), gscale)
    assert np.abs(b["dv"][0] - x.grad.numpy()).max() <= 1e-12
    assert np.abs(b["dp"][0] - z.grad.view(B * T, T).numpy()).max() <= 1e-12
    assert np.abs(b["dsw"][0] - s.grad.numpy()).max() <= 1e-12
    if eps > 0 and w is None:                                    # the part the label is not in gets a gradient
        assert np.abs(b["dp"][0][ref["R"]["is_v"]]).max() > 0 and np.abs(b["dv"][0][ref["R"]["is_p"]]).max() > 0
    if w is not None:                                            # a zero-weight drawing: exact zeros, and real rows under them
        k = int((w == 0).nonzero()[0])
        rows = slice(k * T, (k + 1) * T)
        assert ref["R"]["valid"][rows].any()
        assert not b["dv"][0][rows].any() and not b["dp"][0][rows].any() and not b["dsw"][0][rows].any()
        assert b["zero_v"][rows].all() and b["zero_p"][rows].all() and b["zero_s"][rows].all()


# ------------------------------------------------------------------------------------------------ 2: the float32 restatement passes
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_float32_restatement_passes_the_checker(c):
    t = rp.nll_inputs(c)
    for eps in (0.0, 0.1):
        for kind in R.WEIGHT_KINDS:
            w = R.ext_weight(c, kind)
            rows = R.verify(c, t, eps, w, R.simulate(c, t, eps, w))
            assert all(r is not None and r <= 2.0 for _, r, _ in rows), (eps, kind, rows)


def test_weights_of_the_table_hold_a_zero_and_a_negative():
    for c in CASES:
        wt = R.ext_weight(c, "BT")
        assert bool((wt == 0).any()) and bool((wt < 0).any()) and bool((wt > 0).any())
        wb = R.ext_weight(c, "B")
        assert wb.shape == (c["B"],) and (c["B"] < 2 or (float(wb[0]) < 0 and float(wb[1]) == 0))
    c = next(c for c in CASES if c["B"] == 3)                      # a zero-weight drawing with real rows
    valid = (rp.nll_inputs(c)["label"] != rp.nll_inputs(c)["pad"]).view(c["B"], c["T"])
    assert bool(valid[1].any())


# ------------------------------------------------------------------------------------------------ 3: seeded defects
DEFECT_SETTINGS = {"smooth_over_fills": (0.1, None), "weight_in_denominator": (0.0, "BT"), "dsw_without_eps": (0.1, None),
                   "weight_indexed_by_row": (0.0, "B"), "inv_C_as_inv_V": (0.1, None), "other_part_zero": (0.1, "BT")}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defects_are_caught(defect):
    assert sorted(DEFECT_SETTINGS) == sorted(R.DEFECTS)
    c = next(c for c in CASES if c["name"] == "nll_B2_T36_V514_ld520_x1")
    t = rp.nll_inputs(c)
    eps, kind = DEFECT_SETTINGS[defect]
    w = R.ext_weight(c, kind)
    R.verify(c, t, eps, w, R.simulate(c, t, eps, w))                 # (sound without the defect)
    with pytest.raises(AssertionError, match="tier 1|exact decision"):
        R.verify(c, t, eps, w, R.simulate(c, t, eps, w, defect))


# ------------------------------------------------------------------------------------------------ 4: ABI
def test_loss_block_mirror_matches_the_header_and_the_library():
    """Field order and types from the typedef in include/plank_hip.h; the size from the compiled library itself."""
    hdr = open(os.path.join(REPO, "include", "plank_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} pa_loss_ext;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        if "*" in decl:
            fields.append((decl.rsplit(" ", 1)[1].lstrip("*"), ctypes.c_void_p))
            continue
        kind = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float}[decl.split(" ", 1)[0]]
        fields += [(n.strip(), kind) for n in decl.split(" ", 1)[1].split(",")]
    assert [(n, t) for n, t in L.LossExt._fields_] == fields
    assert [n for n, _ in fields] == ["smoothing", "weight_per_token", "weight", "token_nll", "ext_stats"]
    assert ctypes.sizeof(L.LossExt) == 32 and L.LossExt.weight.offset == 8 and L.LossExt.ext_stats.offset == 24
    lib = ctypes.CDLL(L.LIB_PATH)
    lib.pa_loss_ext_bytes.restype = ctypes.c_int64
    assert lib.pa_loss_ext_bytes() == ctypes.sizeof(L.LossExt)
    for name in ("pa_mixture_nll_fwd_ext", "pa_mixture_nll_bwd_ext", "pa_model_set_loss"):
        assert hasattr(lib, name), name
    assert re.search(r"pa_loss_ext.*?models\.py:219-227", hdr, flags=re.S) or re.search(r"models\.py:219-227.*?pa_loss_ext", hdr, flags=re.S)


# ------------------------------------------------------------------------------------------------ 5: the Python surface's argument checks
@pytest.mark.parametrize("bad", [1.0, -0.1, 1.5, float("nan"), float("inf"), "0.1", True, [0.1]])
def test_build_model_rejects_bad_label_smoothing(bad):
    hp = small_hparams()
    hp["MODEL"]["LABEL_SMOOTHING"] = bad
    with pytest.raises(ValueError, match="LABEL_SMOOTHING"):
        Trainer(hp)


def test_label_smoothing_reaches_the_model_and_defaults_to_off():
    assert Trainer(small_hparams()).model.label_smoothing == 0.0
    hp = small_hparams()
    hp["MODEL"]["LABEL_SMOOTHING"] = 0.1
    t = Trainer(hp)
    assert t.model.label_smoothing == 0.1 and t.hparams_dict["MODEL"]["LABEL_SMOOTHING"] == 0.1


@pytest.mark.parametrize("shape", [(3,), (4, 35), (4, 36, 1), (), (36,), (36, 4)])
def test_bad_loss_weight_shape_raises_without_a_gpu(shape, monkeypatch):
    m = Trainer(small_hparams()).model                            # on the CPU: anything past the argument check would need the device
    monkeypatch.setattr(L, "lib", lambda: pytest.fail("train_step touched the library before checking loss_weight"))
    batch = {"output_label": torch.zeros(4, 36, dtype=torch.int64), "loss_weight": torch.ones(shape)}
    with pytest.raises(ValueError, match="loss_weight"):
        m.train_step(batch)
    batch["loss_weight"] = torch.ones(4, dtype=torch.int64)         # right shape, not a float tensor
    with pytest.raises(ValueError, match="loss_weight"):
        m.train_step(batch)
