"""The reprojection score without a GPU: the host restatement metric.line_overlap_counts (interval algebra)
and the stand-alone host program of tools/overlap_host (the kernel's own core, csrc/overlap_core.h, built by the host compiler with
the address and undefined-behaviour sanitizers) against the unit-cell raster of tests/reprojection_reference.py - integers, so
every comparison is an equality - then the options of the model and the trainer, and the ABI's declaration and binding."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import reprojection_reference as R
from conftest import REPO
from plankassembly_amd import metric as M

TOLS = (0, 1, 3)
MODE_ID = {"ignore": 0, "match": 1, "visible": 2}


def named_checks():
    """(name, a, b, kw, expected or None) for every check of every named case."""
    for name, a, b, bits, checks in R.named_cases():
        for tol, mode, want in checks:
            if mode == "match" and (a[2] is None or b[2] is None):
                continue
            yield name, a, b, dict(end_token=2 ** bits, num_bits=bits, tol=tol, types=mode), want


def generated_checks():
    for name, a, b, bits in R.generated_cases():
        for tol in TOLS:
            for mode in R.MODES:
                yield name, a, b, dict(end_token=2 ** bits, num_bits=bits, tol=tol, types=mode), None


@pytest.fixture(scope="module")
def checks():
    """Every named and generated check with the oracle's counts, computed once."""
    return [(name, a, b, kw, R.line_overlap(a, b, **kw), want) for name, a, b, kw, want in list(named_checks()) + list(generated_checks())]


# -------------------------------------------------------------------------------------------------- the oracle and the host
def test_the_oracle_gives_the_counts_worked_out_by_hand(checks):
    names = {c[0] for c in checks}
    assert {"empty_a", "empty_b", "empty_both", "no_end", "end_at_0", "identical", "other_view", "other_orientation", "c_off_by_1",
            "mirrored_axis", "ends_short_by_tol", "ends_short_by_tol_plus_1", "touching_end_to_end", "b_lines_overlap_each_other",
            "c_minus_1_and_plus_1", "duplicate_on_a", "point", "box", "pad_before_end", "view_3", "type_modes",
            "tol_larger_than_the_line", "bits_11"} <= names
    pinned = 0
    for name, a, b, kw, got, want in checks:
        if want is not None:
            assert got.tolist() == want, (name, kw)
            pinned += 1
    assert pinned >= 50
    assert sum(1 for c in checks if c[0].startswith("gen")) == 40 * 9


def test_identity_and_the_mirrored_axis(checks):
    by = {(c[0], c[3]["tol"], c[3]["types"]): c[4] for c in checks}
    for tol in TOLS:
        r, p, f = R.scores(by["identical", tol, "ignore"])
        assert (r, p, f) == (1.0, 1.0, 1.0)
    assert R.scores(by["mirrored_axis", 1, "ignore"])[2] == 1.0
    assert 0.0 < R.scores(by["mirrored_axis", 0, "ignore"])[2] < 1.0
    assert R.scores(by["empty_both", 1, "ignore"]) == (0.0, 0.0, 0.0)


def test_host_restatement_equals_the_oracle(checks):
    for name, a, b, kw, want, _ in checks:
        got = M.line_overlap_counts(a, b, **kw)
        assert got.dtype == np.int32 and got.tolist() == want.tolist(), (name, kw)
        assert got[0] <= got[1] and got[2] <= got[3], name                         # cov <= len
    with pytest.raises(ValueError):
        M.line_overlap_counts(R.side_of([], with_type=False), R.side_of([]), end_token=512, num_bits=9, types="match")
    with pytest.raises(ValueError):
        M.line_overlap_counts(R.side_of([]), R.side_of([]), end_token=512, num_bits=9, types="hidden")
    with pytest.raises(ValueError):
        M.line_overlap_counts(R.side_of([]), R.side_of([]), end_token=512, num_bits=9, tol=-1)


def test_swapping_the_sides_swaps_the_halves(checks):
    for name, a, b, kw, want, _ in checks:
        if kw["types"] == "visible":
            continue
        got = M.line_overlap_counts(b, a, **kw).tolist()
        assert got == [want[2], want[3], want[0], want[1], want[5], want[4], want[7], want[6]], (name, kw)


def permuted(side, rng):
    """The lines of a side in another order (END and what follows stay)."""
    value, view, typ = (None if x is None else x.copy() for x in side)
    hits = np.nonzero(value == 512)[0]
    n = (int(hits[0]) if len(hits) else len(value)) // 4
    idx = (4 * rng.permutation(n)[:, None] + np.arange(4)[None, :]).reshape(-1)
    for x in (value, view, typ):
        if x is not None:
            x[:4 * n] = x[idx]
    return value, view, typ


def test_permuting_the_lines_changes_nothing(checks):
    rng = np.random.default_rng(77)
    for name, a, b, kw, want, _ in checks:
        if kw["num_bits"] != 9 or kw["tol"] == 3:
            continue
        assert M.line_overlap_counts(permuted(a, rng), b, **kw).tolist() == want.tolist(), (name, kw)
        assert M.line_overlap_counts(a, permuted(b, rng), **kw).tolist() == want.tolist(), (name, kw)
        assert R.line_overlap(permuted(a, rng), permuted(b, rng), **kw).tolist() == want.tolist(), (name, kw)


def test_scores_are_the_numpy_formula_bit_for_bit(checks):
    counts = np.stack([c[4] for c in checks])
    r, p, f = R.scores(counts)
    rec, prec, f1 = M.overlap_scores(torch.from_numpy(counts))
    assert rec.dtype == prec.dtype == f1.dtype == torch.float64
    for got, want in ((rec, r), (prec, p), (f1, f)):
        assert np.array_equal(got.numpy().view(np.int64), want.view(np.int64))
    assert float(f.max()) == 1.0 and float(f.min()) == 0.0 and len(np.unique(f)) > 100


# ---------------------------------------------------------------------------------------------------- the core on the host
def _host_compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise RuntimeError("no host C++ compiler found (set CXX)")


@pytest.fixture(scope="module")
def overlap_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("overlap_host") / "overlap_host")
    src = os.path.join(REPO, "tools", "overlap_host", "main.cpp")
    r = subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _side_text(side):
    value, view, typ = side
    rows = [f"{len(value)} {int(typ is not None)}", " ".join(str(int(v)) for v in value), " ".join(str(int(v)) for v in view)]
    if typ is not None:
        rows.append(" ".join(str(int(v)) for v in typ))
    return "\n".join(rows)


def _run_host(exe, tmp_path, items):
    path = os.path.join(str(tmp_path), "cases.txt")
    with open(path, "w") as f:
        f.write(f"{len(items)}\n")
        for a, b, kw in items:
            f.write(f"{kw['end_token']} {kw['num_bits']} {kw['tol']} {MODE_ID[kw['types']]}\n{_side_text(a)}\n{_side_text(b)}\n")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    return np.asarray([[int(v) for v in ln.split()] for ln in r.stdout.splitlines()], dtype=np.int32).reshape(-1, 8)


def test_host_program_equals_the_oracle(overlap_host, tmp_path, checks):
    got = _run_host(overlap_host, tmp_path, [(a, b, kw) for _, a, b, kw, _, _ in checks])
    assert len(got) == len(checks)
    for row, (name, a, b, kw, want, _) in zip(got, checks):
        assert row.tolist() == want.tolist(), (name, kw)


def test_host_program_at_1024_lines_a_side(overlap_host, tmp_path):
    name, a, b, bits = R.large_case()
    assert len(a[0]) == 4097 and len(b[0]) == 4097
    items = [(a, b, dict(end_token=2 ** bits, num_bits=bits, tol=tol, types=mode)) for tol, mode in ((1, "ignore"), (0, "match"), (3, "visible"))]
    got = _run_host(overlap_host, tmp_path, items)
    for row, (_, _, kw) in zip(got, items):
        want = R.line_overlap(a, b, **kw)
        assert row.tolist() == want.tolist(), kw
        assert want[4] + want[6] == 1024 and want[0] > 1000
    assert got[0][5] + got[0][7] == 1024 and got[2][5] + got[2][7] < 1024          # visible: the hidden lines are not counted


def test_host_program_refuses_what_the_library_refuses(overlap_host, tmp_path):
    one = "1 0\n512\n0\n"
    typed = "1 1\n512\n0\n0\n"
    wide = "4100 0\n" + "1 " * 4100 + "\n" + "0 " * 4100 + "\n"
    for text in (f"1\n512 12 1 0\n{one}{one}", f"1\n512 0 1 0\n{one}{one}", f"1\n512 9 256 0\n{one}{one}", f"1\n512 9 -1 0\n{one}{one}",
                 f"1\n512 9 1 3\n{one}{one}", f"1\n512 9 1 1\n{typed}{one}", f"1\n512 9 1 1\n{one}{typed}", f"1\n512 9 1 0\n{wide}{one}"):
        path = os.path.join(str(tmp_path), "bad.txt")
        with open(path, "w") as f:
            f.write(text)
        r = subprocess.run([overlap_host, path], capture_output=True, text=True)
        assert r.returncode == 2 and r.stdout.strip() == "error", text[:40]
    path = os.path.join(str(tmp_path), "good.txt")
    with open(path, "w") as f:
        f.write(f"1\n512 9 1 1\n{typed}{typed}")
    r = subprocess.run([overlap_host, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["0"] * 8


# -------------------------------------------------------------------------------------------------------------- the options
def test_check_select_accepts_reprojection_and_nothing_else():
    from plankassembly_amd.models import PlankModel
    assert PlankModel._check_select("reprojection") == "reprojection"
    assert PlankModel._check_select("consensus") == "consensus" and PlankModel._check_select(None) is None
    with pytest.raises(ValueError):
        PlankModel._check_select("median")


def _trainer(model=None, data=None, cls=None, **hparams):
    from plankassembly_amd.config import load_cli_config
    from plankassembly_amd.trainer import Trainer
    _, _, hp = load_cli_config(os.path.join(REPO, "configs", "train_complete.yaml"))
    hp["MODEL"].update(NUM_MODEL=64, NUM_HEAD=4, NUM_FEEDFORWARD=128, NUM_ENCODER_LAYERS=1, NUM_DECODER_LAYERS=1, **(model or {}))
    hp["DATA"].update(MAX_INPUT_LENGTH=65, MAX_OUTPUT_LENGTH=36, **(data or {}))
    hp.update(hparams)
    return (cls or Trainer)(hp)


def test_build_model_reads_the_reprojection_keys():
    t = _trainer()
    assert t.model.sample_select is None and (t.model.reprojection_tol, t.model.reprojection_types) == (1, "ignore")
    assert t.reprojection_metric is False
    t = _trainer(dict(NUM_SAMPLES=4, SAMPLE_SELECT="reprojection"))
    assert t.model.sample_select == "reprojection" and (t.model.reprojection_tol, t.model.reprojection_types) == (1, "ignore")
    t = _trainer(dict(NUM_SAMPLES=4, SAMPLE_SELECT="reprojection", REPROJECTION_TOL=0, REPROJECTION_TYPES="visible", SHARE_ENCODER=True,
                      CONSTRAIN_PLANKS=True))
    assert (t.model.reprojection_tol, t.model.reprojection_types) == (0, "visible")
    assert _trainer(dict(REPROJECTION_TYPES="match")).model.reprojection_types == "match"
    bad = [dict(SAMPLE_SELECT="reprojection"),                                       # nothing to choose among
           dict(SAMPLE_SELECT="reprojection", BEAM_SIZE=4),
           dict(NUM_SAMPLES=4, SAMPLE_SELECT="reprojection", BEAM_SIZE=2),
           dict(NUM_SAMPLES=4, SAMPLE_SELECT="median"),
           dict(NUM_SAMPLES=4, SAMPLE_SELECT="reprojection", REPROJECTION_TOL=256),
           dict(NUM_SAMPLES=4, SAMPLE_SELECT="reprojection", REPROJECTION_TOL=-1),
           dict(NUM_SAMPLES=4, SAMPLE_SELECT="reprojection", REPROJECTION_TOL=1.5),
           dict(NUM_SAMPLES=4, SAMPLE_SELECT="reprojection", REPROJECTION_TOL=True),
           dict(NUM_SAMPLES=4, SAMPLE_SELECT="reprojection", REPROJECTION_TYPES="hidden")]
    for model in bad:
        with pytest.raises(ValueError):
            _trainer(model)
    with pytest.raises(ValueError):                                                  # the renderer draws planks of six DOF
        _trainer(dict(NUM_SAMPLES=4, SAMPLE_SELECT="reprojection"), dict(NUM_OUTPUT_DOF=4))
    with pytest.raises(ValueError):                                                  # no type embedding: nothing to match
        _trainer(dict(NUM_SAMPLES=4, SAMPLE_SELECT="reprojection", REPROJECTION_TYPES="match"), dict(NUM_TYPE=0))


def test_reprojection_metric_is_a_validated_hparam():
    from plankassembly_amd.trainer import SidefaceTrainer, reprojection_option
    assert _trainer(REPROJECTION_METRIC=True).reprojection_metric is True
    assert _trainer(REPROJECTION_METRIC=False).reprojection_metric is False
    assert reprojection_option({}) is False
    for v in ("true", 1, "yes"):
        with pytest.raises(ValueError):
            _trainer(REPROJECTION_METRIC=v)
    with pytest.raises(ValueError):                                                  # faces are not lines
        reprojection_option({"REPROJECTION_METRIC": True}, "sideface")
    with pytest.raises(ValueError):
        reprojection_option({"REPROJECTION_METRIC": True}, "line", 4)
    assert reprojection_option({"REPROJECTION_METRIC": False}, "sideface") is False
    assert SidefaceTrainer.device_kind == "sideface"


def test_the_entry_is_declared_and_bound():
    header = open(os.path.join(REPO, "include", "plank_hip.h")).read()
    m = re.search(r"int pa_line_overlap\(([^;]*)\);", header)
    assert m and m.group(1).count(",") == 18                                          # 19 arguments
    lib = open(os.path.join(REPO, "plankassembly_amd", "_lib.py")).read()
    m = re.search(r'"pa_line_overlap": \(I, \[([^\]]*)\]\)', lib)
    assert m and len(m.group(1).split(",")) == 19
    assert "overlap.hip" in __import__("plankassembly_amd.build", fromlist=["SOURCES"]).SOURCES
    for name in ("PA_OVERLAP_IGNORE 0", "PA_OVERLAP_MATCH 1", "PA_OVERLAP_VISIBLE 2", "PA_OVERLAP_MAX_TOL 255"):
        assert f"#define {name}" in header
    from plankassembly_amd import ops
    assert ops.OVERLAP_MODES == {"ignore": 0, "match": 1, "visible": 2}
