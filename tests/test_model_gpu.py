"""Model-level parity on the GPU: plankassembly_amd.PlankModel (HIP path through the C ABI) against
the golden vectors produced by the reference model (tests/golden) and the CPU oracle."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOKEN = types.SimpleNamespace(END=512, PAD=513)


def make(sd, dtype="f32", d=64, h=4, ff=128, ne=2, nd=2, max_in=65, max_out=36, dropout=0.0):
    from plankassembly_amd.models import PlankModel
    m = PlankModel(d, h, ff, dropout, "relu", True, ne, nd, 3, 2, 4, 6, max_in, max_out, 514, TOKEN,
                   compute_dtype=dtype)
    m.load_state_dict(sd)
    return m.cuda()


def to_dev(batch):
    return {k: v.cuda() for k, v in batch.items()}


def test_g1_g2_train_forward_backward_f32(small_fixture):
    sd, batch, g = small_fixture
    m = make(sd).train()
    out = m(to_dev(batch))
    assert abs(out["loss"].item() - float(g["g1::loss"])) < 1e-4
    assert abs(out["accuracy"].item() - float(g["g1::accuracy"])) < 1e-6
    B, S = batch["input_value"].shape
    mem = m.debug_tensor("memory").view(B, S, -1).cpu()
    valid = ~batch["input_mask"]
    assert float((mem[valid] - torch.from_numpy(g["g1::memory"])[valid]).abs().max()) < 1e-4
    hid = m.debug_tensor("hiddens").view(B, -1, 64).cpu()
    assert float((hid - torch.from_numpy(g["g1::hiddens"])).abs().max()) < 1e-4
    out["loss"].backward()
    worst = ("", 0.0)
    for k, p in m.named_parameters():
        ref = torch.from_numpy(g["g2::" + k])
        assert p.grad is not None, k
        err = float((p.grad.cpu() - ref).abs().max())
        scale = float(ref.abs().max())
        rel = err / max(scale, 1e-3)
        if rel > worst[1]:
            worst = (k, rel)
        assert err <= 1e-5 + 1e-4 * scale, (k, err, scale)
    print("worst relative grad error", worst)


def test_g3_fused_adam_step(small_fixture):
    from plankassembly_amd.optim import FusedAdam
    sd, batch, g = small_fixture
    m = make(sd).train()
    opt = FusedAdam(m, lr=1e-4)
    opt.zero_grad()
    m(to_dev(batch))["loss"].backward()
    opt.step()
    # on step 1 the update is lr * g/(|g|+eps): entries with |g| ~ eps are noise-dominated, so
    # compare where the reference gradient is well above eps and bound the rest by lr
    for k, v in m.state_dict().items():
        ref = torch.from_numpy(g["g3::" + k])
        gref = torch.from_numpy(g["g2::" + k]).abs()
        diff = (v.cpu() - ref).abs()
        assert float(diff.max()) <= 2.0001e-4, k
        solid = gref > 1e-5
        if solid.any():
            assert float(diff[solid].max()) < 2e-6, (k, float(diff[solid].max()))


@pytest.mark.parametrize("fixture_name", ["small_fixture", "ragged_fixture"])
def test_prepared_batch_matches_golden_gradients(fixture_name, request):
    """prepare_batch() attaches the encoder packing and the per-table row groupings (segment-sum embedding gradients
    instead of atomics): every gradient must still match the reference's (G2)."""
    sd, batch, g = request.getfixturevalue(fixture_name)
    m = make(sd).train()
    if not m.unpad:
        pytest.skip("PLANK_UNPAD=0: the dense path keeps no packing / groupings")
    pb = m.prepare_batch(batch)
    assert "_groups" in pb and pb["_groups"]["out"] is not None
    out = m(pb)
    assert abs(out["loss"].item() - float(g["g1::loss"])) < 1e-4
    out["loss"].backward()
    for k, p in m.named_parameters():
        if ("g2::" + k) not in g:
            continue
        ref = torch.from_numpy(g["g2::" + k])
        err = float((p.grad.cpu() - ref).abs().max())
        assert err <= 1e-5 + 1e-4 * float(ref.abs().max()), (k, err)


def test_bf16_packed_cross_kv_matches_per_layer_path(small_fixture, monkeypatch):
    """bf16 backward: d(memory) as one GEMM over the packed K/V shadow of all decoder layers vs the per-layer
    accumulating GEMMs - every gradient (the encoder's depend on d(memory)) must agree to bf16 rounding."""
    sd, batch, _ = small_fixture
    grads = []
    for flag in ("1", "0"):
        monkeypatch.setenv("PLANK_CROSS_KV", flag)
        mdl = make(sd, dtype="bf16").train()
        out = mdl(to_dev(batch))
        out["loss"].backward()
        assert (mdl._kvT is not None) == (flag == "1")
        grads.append({k: p.grad.detach().float().cpu().clone() for k, p in mdl.named_parameters()})
    num = den = 0.0
    for k in grads[0]:
        a, b = grads[0][k].flatten(), grads[1][k].flatten()
        num += float((a * b).sum()); den += float(a.norm() * b.norm())
        if k.startswith("encoder") or k.startswith("input_embeddings"):
            assert float((a - b).abs().max()) <= 0.05 * float(b.abs().max()) + 1e-6, k
    assert num / max(den, 1e-30) > 0.999


def test_g7_ragged_sideface_f32(ragged_fixture):
    sd, batch, g = ragged_fixture
    m = make(sd).train()
    out = m(to_dev(batch))
    assert abs(out["loss"].item() - float(g["g1::loss"])) < 1e-4
    hid = m.debug_tensor("hiddens").view(batch["output_value"].shape[0], -1, 64).cpu()
    assert float((hid - torch.from_numpy(g["g1::hiddens"])).abs().max()) < 1e-4
    out["loss"].backward()
    for k in ("input_embeddings.input_value.weight", "input_embeddings.input_view.weight",
              "decoder.layers.1.multihead_attn.in_proj_weight"):
        ref = torch.from_numpy(g["g2::" + k])
        err = float((dict(m.named_parameters())[k].grad.cpu() - ref).abs().max())
        assert err <= 1e-5 + 1e-4 * float(ref.abs().max()), (k, err)
    gt = dict(m.named_parameters())["input_embeddings.input_type.weight"].grad
    assert gt is not None and not gt.any()                  # unused table: zero gradient, no error


def test_train_bf16_close_to_oracle(tiny_fixture):
    """bf16 throughput path vs the f32 CPU oracle on the (untrained) tiny BASELINE config, where the
    gradients carry signal (the briefly-trained small fixture sits at loss 0.01: noise-level grads)."""
    from oracle import plank_oracle as O
    from plankassembly_amd.data import SynthSpec, synth_batch
    sd, _, g = tiny_fixture
    batch = synth_batch(4, SynthSpec(1200, 128, (8, 299), (2, 21), True), seed=int(g["g8::seed"]))
    batch.pop("name")
    cfg = O.OracleCfg(d_model=128, n_head=8, d_ff=256, n_enc=2, n_dec=2, max_input_length=1200, max_output_length=128)
    p = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = O.train_forward(p, cfg, batch)
    ref["loss"].backward()
    m = make(sd, "bf16", 128, 8, 256, 2, 2, 1200, 128).train()
    out = m(to_dev(batch))
    assert abs(out["loss"].item() - float(ref["loss"])) < 2e-2 * float(ref["loss"])
    out["loss"].backward()
    num = den1 = den2 = 0.0
    worst = 1.0
    for k, prm in m.named_parameters():
        r = p[k].grad.double().flatten()
        got = prm.grad.cpu().double().flatten()
        num += float(got @ r); den1 += float(got @ got); den2 += float(r @ r)
        if float(r @ r) > 0:
            worst = min(worst, float(got @ r) / (float(got @ got) ** 0.5 * float(r @ r) ** 0.5 + 1e-30))
    cos = num / (den1 ** 0.5 * den2 ** 0.5)
    print("bf16 grad cosine total", cos, "worst tensor", worst)
    assert cos > 0.995, cos
    assert worst > 0.95, worst


def test_g8_tiny_config_loss_curve(tiny_fixture):
    from plankassembly_amd.data import SynthSpec, synth_batch
    from plankassembly_amd.optim import FusedAdam
    sd, _, g = tiny_fixture
    batch = synth_batch(4, SynthSpec(1200, 128, (8, 299), (2, 21), True), seed=int(g["g8::seed"]))
    batch.pop("name")
    m = make(sd, "f32", 128, 8, 256, 2, 2, 1200, 128).train()
    opt = FusedAdam(m, lr=1e-4)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        out = m(to_dev(batch))
        out["loss"].backward()
        opt.step()
        losses.append(out["loss"].item())
    assert np.allclose(losses, g["g8::losses"], atol=2e-4), (losses, g["g8::losses"])


def test_gradient_accumulation_and_torch_adam(small_fixture):
    """Drop-in semantics: .grad accumulates across backward calls unless zeroed; torch.optim.Adam works."""
    sd, batch, g = small_fixture
    m = make(sd).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    opt.zero_grad()
    m(to_dev(batch))["loss"].backward()
    g1 = m.vocab_head.weight.grad.clone()
    m(to_dev(batch))["loss"].backward()
    assert float((m.vocab_head.weight.grad - 2 * g1).abs().max()) < 1e-6 * max(1.0, float(g1.abs().max()))
    opt.zero_grad()
    m(to_dev(batch))["loss"].backward()
    assert float((m.vocab_head.weight.grad - g1).abs().max()) < 1e-6
    opt.step()
    ref = torch.from_numpy(g["g3::vocab_head.weight"])
    solid = torch.from_numpy(g["g2::vocab_head.weight"]).abs() > 1e-5
    assert float((m.vocab_head.weight.detach().cpu() - ref)[solid].abs().max()) < 2e-6


def test_dropout_training_runs_and_is_stochastic(small_fixture):
    sd, batch, _ = small_fixture
    m = make(sd, dropout=0.2).train()
    l1 = m(to_dev(batch))["loss"]
    l1.backward()
    l2 = m(to_dev(batch))["loss"]
    assert torch.isfinite(l1) and torch.isfinite(l2) and abs(l1.item() - l2.item()) > 1e-6
    assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    m.eval()


# ------------------------------------------------------------------------------------------ greedy decode
@pytest.mark.parametrize("graph", [False, True])
def test_g4_greedy_decode_token_exact(small_fixture, graph):
    import plankassembly_amd.decode as D
    sd, batch, g = small_fixture
    m = make(sd).eval()
    m._ensure_handle()
    m._decoder = D.GreedyDecoder(m, use_graph=graph, check_every=5)
    with torch.no_grad():
        out = m(to_dev(batch))
    assert np.array_equal(out["samples"].cpu().numpy(), g["g4::samples"])       # bit-exact tokens
    assert np.array_equal(out["attach"].cpu().numpy(), g["g4::attach"])
    assert (out["attach"] >= 0).any()
    for i, (p, q) in enumerate(zip(out["predicts"], out["groundtruths"])):
        assert np.array_equal(p.cpu().numpy(), g[f"g4::predict{i}"])
        assert np.array_equal(q.cpu().numpy(), g[f"g4::groundtruth{i}"])
    # a second call (graph reuse, new batch tensors) gives the same answer
    with torch.no_grad():
        out2 = m(to_dev(batch))
    assert torch.equal(out2["samples"], out["samples"]) and torch.equal(out2["attach"], out["attach"])


def test_g7_greedy_decode_ragged_sideface(ragged_fixture):
    sd, batch, g = ragged_fixture
    m = make(sd).eval()
    with torch.no_grad():
        out = m(to_dev(batch))
    assert np.array_equal(out["samples"].cpu().numpy(), g["g4::samples"])
    assert np.array_equal(out["attach"].cpu().numpy(), g["g4::attach"])


def test_greedy_decode_no_early_stop_matches_oracle(small_fixture):
    """Run all max_output_length steps (the decode benchmark mode) and compare with the oracle."""
    from oracle import plank_oracle as O
    import plankassembly_amd.decode as D
    sd, batch, _ = small_fixture
    cfg = O.OracleCfg(d_model=64, n_head=4, d_ff=128, n_enc=2, n_dec=2, max_input_length=65, max_output_length=36)
    with torch.no_grad():
        s_ref, a_ref = O.greedy_decode_cached(sd, cfg, batch, early_stop=False)
    m = make(sd).eval()
    m._ensure_handle()
    dec = D.GreedyDecoder(m)
    s, a = dec.run(to_dev(batch), early_stop=False)
    assert s.shape == (4, 36)
    assert torch.equal(s.cpu(), s_ref) and torch.equal(a.cpu(), a_ref)


def test_greedy_decode_bf16_mostly_agrees(small_fixture):
    sd, batch, g = small_fixture
    m = make(sd, "bf16").eval()
    with torch.no_grad():
        out = m(to_dev(batch))
    ref = torch.from_numpy(g["g4::samples"])
    n = min(ref.shape[1], out["samples"].shape[1])
    agree = (out["samples"].cpu()[:, :n] == ref[:, :n]).float().mean().item()
    assert agree > 0.9, agree


# ------------------------------------------------------------------------------------------ bf16 shadow staleness
def test_bf16_shadow_follows_torch_adam_and_load_state_dict(small_fixture):
    """The bf16 GEMM-operand shadows (weights, W^T, packed cross K/V) must follow parameter updates that do not go
    through FusedAdam: torch.optim.Adam steps and load_state_dict after a first forward (INTEGRATION.md drop-in path)."""
    sd, batch, _ = small_fixture
    gb = to_dev(batch)
    m = make(sd, dtype="bf16").train()
    opt = torch.optim.Adam(m.parameters(), lr=5e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        out = m(gb)
        out["loss"].backward()
        opt.step()
        losses.append(out["loss"].item())
    # a model that keeps computing on the initial weights reports the same loss every step
    assert max(losses) - min(losses) > 1e-3, losses
    # the loss of the updated weights, seen by a fresh module that casts its shadow from scratch
    fresh = make({k: v.detach().cpu() for k, v in m.state_dict().items()}, dtype="bf16").train()
    a, b = m(gb)["loss"].item(), fresh(gb)["loss"].item()
    assert abs(a - b) <= 1e-3 * max(1.0, abs(b)), (a, b)
    # load_state_dict after a forward: the next forward must see the loaded weights
    m.load_state_dict(sd)
    ref = make(sd, dtype="bf16").train()
    a, b = m(gb)["loss"].item(), ref(gb)["loss"].item()
    assert abs(a - b) <= 1e-3 * max(1.0, abs(b)), (a, b)
    m.eval()
    with torch.no_grad():
        m.vocab_head.bias.add_(0.0)                      # in-place touch through the parameter also invalidates
    assert m._param_version() != m._shadow_version


# ------------------------------------------------------------------------------------------ batch preparation kernels
@pytest.mark.parametrize("kind", ["headline", "sideface"])
def test_prepare_batch_groupings_match_the_torch_statement(kind):
    """pa_pack_rows (one launch) + pa_group_rows (one launch, all eight tables) against argsort / bincount: identical
    `order` (stable: ties in token order) and `seg` for every table, incl. the batch without input_type and empty rows."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import large_cases as LC
    from plankassembly_amd.models import INPUT_KEYS, group_rows_by_id
    c = LC.CASES[kind]
    batch = LC.case_batch(c, batch_size=16)
    from plankassembly_amd.models import PlankModel
    m = PlankModel(64, 4, 128, 0.0, "relu", True, 1, 1, 3, 2, 4, 6, c["max_in"], c["max_out"], 514, TOKEN).cuda()
    if not m.unpad:
        pytest.skip("PLANK_UNPAD=0: the dense path keeps no packing / groupings")
    pb = m.prepare_batch(batch)
    cu, rowmap, n_valid = pb["_pack"]
    valid = (~batch["input_mask"]).flatten().nonzero().flatten()
    assert n_valid == valid.numel() and torch.equal(rowmap[:n_valid].cpu().long(), valid)
    sel = rowmap[:n_valid].long()
    for j, key in enumerate(INPUT_KEYS):
        grp = pb["_groups"]["in"][j]
        if key not in batch:
            assert grp is None
            continue
        rows = m._shapes[f"input_embeddings.{key}.weight"][0]
        o_ref, s_ref = group_rows_by_id(pb[key].reshape(-1)[sel], rows)
        assert torch.equal(grp[0], o_ref) and torch.equal(grp[1], s_ref), key
    ov = pb["output_value"]
    Bq, Tq = ov.shape
    tpos = torch.arange(1, Tq, device="cuda")
    rows_bt = (torch.arange(Bq, device="cuda")[:, None] * Tq + tpos[None, :]).reshape(-1)
    prev = (tpos - 1)[None, :].expand(Bq, -1).reshape(-1)
    refs = [group_rows_by_id(ov[:, :-1].reshape(-1), 514, rows_bt), group_rows_by_id(prev % 6, 6, rows_bt),
            group_rows_by_id(prev // 6, (Tq + 5) // 6, rows_bt)]
    for (o, s_), (o_ref, s_ref) in zip(pb["_groups"]["out"], refs):
        assert torch.equal(o, o_ref) and torch.equal(s_, s_ref)


@pytest.mark.parametrize("graph", [False, True])
def test_two_lane_decode_equals_single_lane(small_fixture, graph):
    """Batches of >= 32 samples decode as two half-batches on two streams inside one graph (decode.GreedyDecoder lanes):
    tokens and attach must equal the single-stream result bit for bit, with early stop and at full length."""
    import plankassembly_amd.decode as D
    from plankassembly_amd.data import SynthSpec, synth_batch
    sd, _, _ = small_fixture
    batch = synth_batch(40, SynthSpec(65, 36, (0, 15), (2, 5), True), seed=11)
    batch.pop("name")
    m = make(sd).eval()
    m._ensure_handle()
    gb = to_dev(batch)
    for early in (True, False):
        one = D.GreedyDecoder(m, use_graph=graph, lanes=1, strict_graph=True)
        two = D.GreedyDecoder(m, use_graph=graph, lanes=2, strict_graph=True)
        with torch.no_grad():
            s1, a1 = one.run(gb, early_stop=early)
            s2, a2 = two.run(gb, early_stop=early)
            s3, a3 = two.run(m.prepare_batch(batch), early_stop=early)      # prepared input, graph reused
        assert two._active == 2 and one._active == 1
        assert torch.equal(s1, s2) and torch.equal(a1, a2)
        assert torch.equal(s1, s3) and torch.equal(a1, a3)
        del one, two
