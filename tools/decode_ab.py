"""Bit-for-bit A/B of the decode step between two builds of the library (the method of profiles/decode_dispatch_refactor.txt, section 2).

    python tools/decode_ab.py LIB_A LIB_B [OUT_DIR]        (OUT_DIR: where the children's tensors are kept; default a temporary directory)

A library that lies in a checkout's plankassembly_amd/ is run through that checkout's own Python binding (two commits may differ in
the symbols they export); any other path is loaded by this tree's binding through PLANK_HIP_LIB.
For each library and each switch bundle a fresh child process - the switches are read once per process -
decodes a small seeded model (d_model 512, 8 heads, d_ff 512, 2 + 2 layers, S 40 with ragged lengths, Tmax 12) four ways: greedy,
beam K 3, sampling N 2 with a seed, and a forced prefix with its per-position log-probabilities; at B 4, at B 200 once (the default
bf16 bundle: the absorbed self-attention's threshold) and at B 40 with lanes=2.  A child writes tokens, attach, scores and prefix_lp to
OUT_DIR/<a|b>_<bundle>.pt; this process requires the two builds' tensors to be equal byte for byte.  Every child runs under its own
time limit and the first failure ends the run."""
import os
import subprocess
import sys
import tempfile
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S_IN, TMAX = 40, 12
BUNDLES = {
    "default_bf16": ("bf16", {}),
    "default_f32": ("f32", {}),
    "MQ=0": ("bf16", {"PLANK_DECODE_MQ": "0"}),
    "FOLD_LN=0": ("bf16", {"PLANK_DECODE_FOLD_LN": "0"}),
    "FOLD_LN=0_f32": ("f32", {"PLANK_DECODE_FOLD_LN": "0"}),
    "F32_RESID=0": ("bf16", {"PLANK_DECODE_F32_RESID": "0"}),
    "MQ_SELF_BF16=1": ("bf16", {"PLANK_DECODE_MQ_SELF_BF16": "1"}),
}


def small_model(dtype):
    from plankassembly_amd.models import PlankModel
    torch.manual_seed(20)
    token = types.SimpleNamespace(END=512, PAD=513)
    m = PlankModel(512, 8, 512, 0.0, "relu", True, 2, 2, 3, 2, 4, 6, S_IN + 1, TMAX, 514, token, compute_dtype=dtype)
    with torch.no_grad():                                       # (wider heads than the default init: the rows take different tokens)
        m.vocab_head.weight.mul_(8.0)
        m.pointer_head.weight.mul_(8.0)
    m = m.cuda().eval()
    m._ensure_handle()
    m._refresh_shadow()
    return m


def ragged_batch(B):
    from plankassembly_amd.data import SynthSpec, synth_batch
    b = synth_batch(B, SynthSpec(S_IN + 1, TMAX, (1, 10), (1, 1), True), seed=7 + B)
    b.pop("name")
    return {k: v.cuda() for k, v in b.items()}


def child(dtype, out, b200):
    pkg = os.path.dirname(os.environ["PLANK_HIP_LIB"])
    sys.path.insert(0, os.path.dirname(pkg) if os.path.basename(pkg) == "plankassembly_amd" else REPO)
    import plankassembly_amd.decode as D
    m = small_model(dtype)
    res = {}
    sizes = [(4, 1), (40, 2)] + ([(200, 1)] if b200 else [])
    with torch.no_grad():
        for B, lanes in sizes:
            gb, tag = ragged_batch(B), f"B{B}_lanes{lanes}"
            dec = D.GreedyDecoder(m, lanes=lanes)
            s, a = dec.run(gb, early_stop=False)
            assert dec._active == lanes
            res[tag + "_greedy"] = (s, a)
            if lanes == 2:
                continue
            prefix = {"tokens": torch.randint(0, 512, (B, 5), generator=torch.Generator().manual_seed(B))}
            s, a = dec.run(gb, early_stop=False, prefix=prefix)
            res[tag + "_prefix"] = (s, a, dec.last_prefix_scores, dec.last_prefix_logprobs)
            r = D.BeamDecoder(m, 3).run(gb, early_stop=False)
            res[tag + "_beam"] = (r["beam_tokens"], r["beam_attach"], r["scores"])
            r = D.SampleDecoder(m, 2, temperature=1.3, top_k=50, top_p=0.95, seed=11).run(gb, early_stop=False)
            res[tag + "_sample"] = (r["sample_tokens"], r["sample_attach"], r["scores"])
    torch.cuda.synchronize()
    torch.save({k: [t.cpu().contiguous() for t in v] for k, v in res.items()}, out)


def raw(t):
    return t.contiguous().view(-1).view(torch.uint8)


def main():
    libs, out_dir = [os.path.abspath(p) for p in sys.argv[1:3]], (sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp())
    os.makedirs(out_dir, exist_ok=True)
    bad = 0
    for name, (dtype, switches) in BUNDLES.items():
        got = []
        for side, lib in zip("ab", libs):
            env = {k: v for k, v in os.environ.items() if not k.startswith("PLANK_DECODE_")}
            env.update(switches, PLANK_HIP_LIB=lib)
            out = os.path.join(out_dir, f"{side}_{name}.pt")
            r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", dtype, out,
                                str(int(name == "default_bf16"))], env=env, cwd=REPO)
            if r.returncode != 0:
                sys.exit(f"{name}: child of {lib} ended with status {r.returncode}: nothing further is started")
            got.append(torch.load(out))
        assert sorted(got[0]) == sorted(got[1])
        for key in sorted(got[0]):
            same = all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(raw(x), raw(y)) for x, y in zip(got[0][key], got[1][key]))
            distinct = len({tuple(row.tolist()) for row in got[0][key][0].reshape(got[0][key][0].shape[0], -1)})
            print(f"{name:16s} {key:22s} {'identical' if same else 'DIFFERENT'}   ({distinct} distinct rows of {got[0][key][0].shape[0]})")
            bad += not same
    print("decode_ab:", "every byte equal" if not bad else f"{bad} results differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        child(sys.argv[2], sys.argv[3], sys.argv[4] == "1")
    else:
        main()
