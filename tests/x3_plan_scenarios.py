"""Scenarios of the bf16x3 cut plan (csrc/gemm.hip plan_split3 / plan_group_split3 / commit_split3; DESIGN.md "bf16x3 plan"):
ordered lists of calls at the C ABI - pa_gemm_split_config, pa_gemm_split_reserve, pa_gemm_split_cache_use, pa_gemm, pa_gemm_group -
and two drivers that turn a scenario into one entry per call:

  real_run   on the GPU: every call really runs, the inner argument blocks come from pa_gemm_record / pa_gemm_recorded;
  dry_run    without a GPU: pa_gemm / pa_gemm_group are replaced by pa_gemm_split_plan(.., commit = 1, ..) over made-up addresses
             (the plan never dereferences a pointer; config / reserve / cache_use only touch the host-side context).

An entry of a GEMM call holds the differences of the process counters (taken, declined, reused, made_hits, cache_hits), the status,
and every inner argument block with A, B and aux written as [region, byte offset] - region "scratch", "cache" or the name of the
caller's own buffer - next to M, N, K, lda, ldb, sA, sB, splitk, splitk_defer.  An entry of a reserve call holds the image's
[region, offset] (null: no image) and its parts pattern.

tests/golden/x3_plan.json was recorded with `python tests/x3_plan_scenarios.py --record` on an MI355X against a library built
from the commit BEFORE the plan functions existed (PLANK_HIP_LIB selects the library; that commit cannot record without a device:
its cut launch fails before the inner GEMM is recorded).  This module therefore binds the few entry points it needs itself and
asks for pa_gemm_split_plan only in the dry driver.

A parts-pattern mismatch between a producer-made image and its consumer cannot be reached through the public entries: every image
of the segment's list has pattern 1 and every image of the forward's list pattern 0, which is also what their consumers cut.  The
scenario "reserve" has the reachable neighbour instead: a made image whose key (rows) does not match the consuming GEMM.
"""
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "x3_plan.json")
if REPO not in sys.path:
    sys.path.insert(0, REPO)

KB = 1024
CACHE_HEAD = 32768                                             # csrc/gemm.hip SPLIT_CACHE_HEAD: the device copy of the refresh job table
PA_F32 = 0


def G(A, B, Cm, M, N, K, akc=True, bkc=True, **kw):
    """One pa_gemm call (or group member): operands as (buffer name, byte offset)."""
    d = dict(A=A, B=B, C=Cm, M=M, N=N, K=K, akc=akc, bkc=bkc)
    d.update(kw)
    return d


def _img(rows, cols):
    return (rows * cols * 6 + 255) // 256 * 256


def _linear(x, w, y, rows=64, din=64, dout=64, **kw):           # y = x w^T: both operands k-contiguous
    return ("gemm", G((x, 0), (w, 0), (y, 0), rows, dout, din, **kw))


def _dx(dy, wt, dx, rows=64, din=64, dout=64, **kw):            # dx = dy w over w^T [din][dout]: both k-contiguous
    return ("gemm", G((dy, 0), (wt, 0), (dx, 0), rows, din, dout, **kw))


def _dw(dy, x, dw, rows=64, din=64, dout=64, **kw):             # dw = dy^T x: the contraction index strided in both
    return G((dy, 0), (x, 0), (dw, 0), dout, din, rows, akc=False, bkc=False, **kw)


def scenarios():
    """name -> dict(scratch, cache, buffers {name: bytes}, calls).  (Groups have at least two members: pa_gemm_split_plan plans a
    single block as pa_gemm would.)  Shapes from {64, 128, 192, 256} plus the odd values that make a
    call decline, 8-row operands where a list has to fill up, scratch buffers of 64 KB .. 1 MB so that every overflow path is reached."""
    S = {}
    big = 256 * 256 * 4
    # 1. the four layouts, plain mode
    S["layouts"] = dict(scratch=256 * KB, buffers=dict(a=big, b=big, c=big), calls=[("config", 1)] + [
        ("gemm", G(("a", 0), ("b", 0), ("c", 0), 128, 64, 192, akc=akc, bkc=bkc))
        for akc, bkc in ((True, True), (True, False), (False, False), (False, True))] + [("config", 0)])
    # 2. every reason to decline (each call runs exact f32)
    S["declines"] = dict(scratch=256 * KB, buffers=dict(a=big, b=big, c=big, g=big, lp=big), calls=[
        ("config", 1),
        ("gemm", G(("a", 0), ("b", 0), ("c", 0), 64, 64, 72)),                                        # K % 64 != 0, both k-contiguous
        ("gemm", G(("a", 0), ("b", 0), ("c", 0), 100, 64, 64, akc=False, bkc=False)),                 # columns of A no multiple of 8
        ("gemm", G(("a", 0), ("b", 0), ("c", 0), 64, 64, 64, lda=66)),                                # leading dimension no multiple of 4
        ("gemm", G(("a", 8), ("b", 0), ("c", 0), 64, 64, 64)),                                        # A 8 bytes off a 16-byte boundary
        ("gemm", G(("a", 0), ("b", 0), ("c", 0), 64, 64, 64, C_lp=("lp", 0), ldc_lp=64)),             # C_lp set
        ("gemm", G(("a", 0), ("b", 0), ("c", 0), 64, 60, 64, aux=("g", 0))),                          # aux with N % 8 != 0
        ("gemm", G(("a", 0), ("b", 0), ("c", 0), 64, 64, 64, splitk=2)),                              # splitk > 1 without ws
        ("gemm", G(("a", 0), ("b", 0), ("c", 0), 256, 64, 256)),                                      # cuts larger than the scratch
        ("gemm", G(("a", 0), ("b", 0), ("c", 0), 64, 64, 64)),                                        # (and one that is taken)
        ("config", 0)])
    # 3. declined with a deferred split-K: the exact kernel writes 2 slabs where the x3 tiling counts 3 (memset branch), then 2 of 2
    S["declined_deferred"] = dict(scratch=512 * KB, buffers=dict(a=big, b=big, c=big, ws=big), calls=[
        ("config", 1),
        ("gemm", G(("a", 0), ("b", 0), ("c", 0), 100, 64, 64, akc=False, bkc=False, splitk=3, defer=1, ws=("ws", 0))),
        ("gemm", G(("a", 0), ("b", 0), ("c", 0), 100, 64, 128, akc=False, bkc=False, splitk=2, defer=1, ws=("ws", 0))),
        ("gemm", G(("a", 0), ("b", 0), ("c", 0), 128, 64, 256, akc=False, bkc=False, splitk=4, defer=1, ws=("ws", 0))),   # (taken)
        ("config", 0)])
    # 4. batches: a shared A, a shared B, and batched operands with a gate
    S["batches"] = dict(scratch=512 * KB, buffers=dict(a=big, b=big, c=big, g=big), calls=[
        ("config", 1),
        ("gemm", G(("a", 0), ("b", 0), ("c", 0), 64, 64, 64, batch=3, sA=0)),
        ("gemm", G(("a", 0), ("b", 0), ("c", 0), 64, 64, 128, batch=3, sB=0, bkc=False)),
        ("gemm", G(("a", 0), ("b", 0), ("c", 0), 64, 64, 64, batch=2, aux=("g", 0), aux_scale=1.25)),
        ("config", 0)])
    # 5. the forward keeps its Linear inputs until 3/4 of the scratch is used; an overflow drops them and closes the list
    xs = {f"x{i}": 64 * 64 * 4 for i in range(9)}
    S["forward_retain"] = dict(scratch=256 * KB, buffers=dict(w=big, y=big, xl=big, **xs), calls=[("config", 3)] + [
        _linear(f"x{i}", "w", "y") for i in range(9)] + [                                             # x0 .. x6 kept, x7 and x8 cut only
        _linear("x0", "w", "y"),                                                                      # past the 3/4 mark: cut again, its older image stays     
        ("gemm", G(("xl", 0), ("w", 0), ("y", 0), 128, 64, 192)),                                     # does not fit behind the images: list dropped and closed
        _linear("x1", "w", "y"),                                                                      # closed: not kept any more
        ("reserve", "x2", 64, 64, 64),                                                                # closed: NULL
        ("config", 0), ("config", 3), _linear("x1", "w", "y"), ("config", 0)])                        # the next forward opens it again
    # 5b. the 129th image of a forward: 126 producer-made images, then GEMMs keep the 127th and 128th and only cut the 129th
    S["forward_129"] = dict(scratch=1024 * KB, buffers=dict(xs=140 * 2048, w=big, y=big), calls=[("config", 3)] + [
        ("reserve", ("xs", 2048 * i), 8, 64, 64) for i in range(126)] + [
        ("gemm", G(("xs", 2048 * i), ("w", 0), ("y", 0), 8, 8, 64)) for i in (126, 127, 128)] + [
        ("reserve", ("xs", 2048 * 129), 8, 64, 64), ("config", 0)])
    # 6. backward segments after a forward: dX GEMMs keep dY, the grouped dW launch finds dY alone / X alone / both / neither;
    #    then an overflow that drops the segment's images only, and one that drops the forward's too
    acts = {k: 64 * 64 * 4 for k in ("xa", "xb", "xc", "dya", "dyb", "dyc", "dyd")}
    S["segment_retain"] = dict(scratch=256 * KB, buffers=dict(w=big, wt=big, y=big, dx=big, big1=big, big2=big, ws=big, odd=big,
                                                              dw0=big, dw1=big, dw2=big, dw3=big, **acts), calls=[
        ("config", 3), _linear("xa", "w", "y"), _linear("xb", "w", "y"), ("config", 0),
        ("config", 2), _dx("dya", "wt", "dx"), _dx("dyb", "wt", "dx"),
        ("group", [_dw("dya", "xa", "dw0"), _dw("dyb", "xc", "dw1"), _dw("dyc", "xb", "dw2"), _dw("dyd", "xc", "dw3")]),
        ("group", [_dw("dya", "xa", "dw0"), G(("odd", 0), ("xa", 0), ("dw1", 0), 100, 64, 64, akc=False, bkc=False)]),   # finds both images of its
                                                                                                      # first member, then declines: nothing reused
        ("gemm", _dw("dya", "xa", "dw0")),                                                            # the lone weight gradient: both found
        ("gemm", _dw("dya", "xb", "dw0", splitk=2, defer=1, ws=("ws", 0))),                           # .. through deferred split-K slabs
        _dx("dyc", "wt", "dx"),
        ("gemm", G(("big1", 0), ("w", 0), ("y", 0), 128, 64, 128)),                                   # drops the segment's images only
        ("group", [_dw("dya", "xa", "dw0"), _dw("dyd", "xb", "dw1")]),                                # dY gone, X still found
        ("gemm", G(("big2", 0), ("w", 0), ("y", 0), 128, 64, 192)),                                   # drops the forward's images too
        ("group", [_dw("dya", "xa", "dw0"), _dw("dyd", "xc", "dw1")]),                                # neither
        ("config", 0),
        ("config", 1), ("gemm", _dw("dya", "xa", "dw0")), ("config", 0)])                             # plain mode forgets the forward
    # 6b. the 17th image of a segment: 15 made by producers, the 16th kept by a GEMM, the 17th only cut, a 17th producer refused
    S["segment_17"] = dict(scratch=256 * KB, buffers=dict(xs=20 * 2048, w=big, y=big), calls=[("config", 2)] + [
        ("reserve", ("xs", 2048 * i), 8, 64, 64) for i in range(15)] + [
        ("gemm", G(("xs", 2048 * i), ("w", 0), ("y", 0), 8, 8, 64)) for i in (15, 16)] + [
        ("reserve", ("xs", 2048 * 17), 8, 64, 64), ("config", 0)])
    # 7. pa_gemm_split_reserve in modes 3 and 2: made and found, made under another key (not used), no room (NULL)
    S["reserve"] = dict(scratch=256 * KB, buffers=dict(w=big, wt=big, y=big, dx=big, dw0=big, dw1=big, xk=big, **acts), calls=[
        ("config", 3),
        ("reserve", "xa", 64, 64, 64), _linear("xa", "w", "y"),                                       # found: no cut of A
        ("reserve", "xb", 64, 64, 64), _linear("xb", "w", "y", rows=32),                              # other rows: not used, cut
        ("reserve", "xk", 512, 64, 64),                                                               # past 3/4 of the scratch: NULL
        ("config", 0), ("config", 2),
        ("reserve", "dya", 64, 64, 64), _dx("dya", "wt", "dx"),                                       # found
        ("group", [_dw("dya", "xa", "dw0"), _dw("dyb", "xb", "dw1")]),                                # the made dY and the made X serve the weight gradient
        ("reserve", "xk", 1024, 64, 64),                                                              # past 7/8 of the scratch: NULL
        ("config", 0)])
    # 8. the weight-image cache: a miss cut into the cache, a hit, a second miss, then a full cache (cut into the scratch)
    S["cache"] = dict(scratch=256 * KB, cache=CACHE_HEAD + 2 * _img(64, 64) + 128, buffers=dict(
        w1=big, w2=big, w3=big, y=big, **acts), calls=[
        ("config", 3), ("cache_use", 1),
        _linear("xa", "w1", "y"), _linear("xb", "w1", "y"), _linear("xa", "w2", "y"), _linear("xb", "w3", "y"),
        _linear("xc", "w2", "y", splitk=2),                                                           # declined (no ws) behind a cache hit
        ("cache_use", 0), _linear("xa", "w1", "y"), ("config", 0)])
    # 9. a grouped launch that declines - no room, then an ineligible member - and the single calls its caller falls back to
    S["group_declines"] = dict(scratch=64 * KB, buffers=dict(dw0=big, dw1=big, odd=big, **acts), calls=[
        ("config", 2),
        ("group", [_dw("dya", "xa", "dw0"), _dw("dyb", "xb", "dw1")]),                                # 96 KB of cuts, 64 KB of scratch
        ("gemm", _dw("dya", "xa", "dw0")), ("gemm", _dw("dyb", "xb", "dw1")),
        ("group", [_dw("dya", "xa", "dw0", rows=32), G(("odd", 0), ("xa", 0), ("dw1", 0), 100, 64, 32, akc=False, bkc=False)]),
        ("gemm", _dw("dya", "xa", "dw0", rows=32)),
        ("gemm", G(("odd", 0), ("xa", 0), ("dw1", 0), 100, 64, 32, akc=False, bkc=False)),
        ("config", 0)])
    for s in S.values():
        s.setdefault("cache", 0)
    return S


# ------------------------------------------------------------------------------------------------------------------- the library
def load_lib(dry):
    """The library under PLANK_HIP_LIB (default: the tree's), with the signatures the drivers use (torch first: one HIP runtime)."""
    import torch                                               # noqa: F401
    from plankassembly_amd import _lib as L
    lib = C.CDLL(L.LIB_PATH)
    P, I, I64 = C.c_void_p, C.c_int32, C.c_int64
    sig = {"pa_gemm": (I, [P, P]), "pa_gemm_group": (I, [P, I, P]), "pa_gemm_split_config": (I, [I, P, I64]),
           "pa_gemm_split_stats": (I, [P, I]), "pa_gemm_split_reused": (I64, []), "pa_gemm_split_made_hits": (I64, []),
           "pa_gemm_split_cache_hits": (I64, []), "pa_gemm_split_reserve": (P, [P, I, I, I, P]),
           "pa_gemm_split_cache_create": (I, [P, I64, P]), "pa_gemm_split_cache_destroy": (None, [P]),
           "pa_gemm_split_cache_use": (I, [P]), "pa_gemm_record": (I, [I]), "pa_gemm_recorded": (I, [P, I]),
           "pa_gemm_effective_splitk": (I, [I, I, I])}
    if dry:
        sig["pa_gemm_split_plan"] = (I, [P, I, I, P])
        sig["pa_gemm_plan"] = (I, [P, P, P])
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def _counters(lib):
    out = (C.c_int64 * 2)()
    lib.pa_gemm_split_stats(out, 0)
    return (int(out[0]), int(out[1]), int(lib.pa_gemm_split_reused()), int(lib.pa_gemm_split_made_hits()),
            int(lib.pa_gemm_split_cache_hits()))


COUNTERS = ("taken", "declined", "reused", "made_hits", "cache_hits")


class _Space:
    """Addresses of a scenario's regions: base[region] (256-byte aligned) and bytes[region]."""

    def __init__(self, sc, base_of):
        self.bytes = dict(sc["buffers"], scratch=sc["scratch"])
        if sc["cache"]:
            self.bytes["cache"] = sc["cache"]
        self.base = {k: base_of(k, n) for k, n in self.bytes.items()}

    def ptr(self, ref):
        if ref is None:
            return None
        name, off = (ref, 0) if isinstance(ref, str) else ref
        return self.base[name] + off

    def where(self, ptr):
        if not ptr:
            return None
        for k, b in self.base.items():
            if b <= ptr < b + self.bytes[k]:
                return [k, ptr - b]
        raise AssertionError(f"address {ptr:#x} lies in no region of the scenario")


def gemm_args(L, sp, g):
    """The pa_gemm_args block of a call dict (strides and leading dimensions default to the dense ones)."""
    M, N, K, nb = g["M"], g["N"], g["K"], g.get("batch", 1)
    a = L.GemmArgs()
    a.A, a.B, a.C = sp.ptr(g["A"]), sp.ptr(g["B"]), sp.ptr(g["C"])
    a.aux, a.ws, a.C_lp = sp.ptr(g.get("aux")), sp.ptr(g.get("ws")), sp.ptr(g.get("C_lp"))
    a.M, a.N, a.K = M, N, K
    a.lda = g.get("lda", K if g["akc"] else M)
    a.ldb = g.get("ldb", K if g["bkc"] else N)
    a.ldc, a.ldaux, a.ldc_lp = N, N, g.get("ldc_lp", 0)
    a.batch = nb
    a.sA, a.sB = g.get("sA", M * K if nb > 1 else 0), g.get("sB", N * K if nb > 1 else 0)
    a.sC = a.sAux = M * N if nb > 1 else 0
    a.a_kcontig, a.b_kcontig = int(g["akc"]), int(g["bkc"])
    a.in_dtype = a.out_dtype = PA_F32
    a.alpha, a.aux_scale = 1.0, g.get("aux_scale", 1.0)
    a.splitk, a.splitk_defer = g.get("splitk", 1), g.get("defer", 0)
    return a


def _block(sp, b):
    return dict(A=sp.where(b.A), B=sp.where(b.B), aux=sp.where(b.aux), M=b.M, N=b.N, K=b.K, lda=b.lda, ldb=b.ldb,
                sA=b.sA, sB=b.sB, splitk=b.splitk, splitk_defer=b.splitk_defer)


def _run(lib, L, sc, sp, cache_buf, do_gemms, do_reserved=None):
    """The calls of one scenario; do_gemms(entry index, kind, arg blocks, call dicts) -> (status, inner blocks) runs or plans a
    GEMM call."""
    cache = C.c_void_p()
    if sc["cache"]:
        assert lib.pa_gemm_split_cache_create(C.c_void_p(cache_buf), sc["cache"], C.byref(cache)) == 0
    lib.pa_gemm_split_stats(None, 1)
    out = []
    try:
        for call in sc["calls"]:
            kind = call[0]
            if kind == "config":
                on = call[1]
                assert lib.pa_gemm_split_config(on, C.c_void_p(sp.base["scratch"]) if on else None, sc["scratch"] if on else 0) == 0
                out.append(dict(call="config", mode=on))
            elif kind == "cache_use":
                assert lib.pa_gemm_split_cache_use(cache if call[1] else None) == 0
                out.append(dict(call="cache_use", on=call[1]))
            elif kind == "reserve":
                _, src, rows, cols, ld = call
                pat = C.c_int32(-1)
                ptr = lib.pa_gemm_split_reserve(C.c_void_p(sp.ptr(src)), rows, cols, ld, C.byref(pat))
                if ptr and do_reserved:
                    do_reserved(ptr, src, rows, cols, ld, pat.value)
                out.append(dict(call="reserve", image=sp.where(ptr), pat=pat.value if ptr else None))
            else:
                gs = [call[1]] if kind == "gemm" else call[1]
                blocks = (L.GemmArgs * len(gs))(*[gemm_args(L, sp, g) for g in gs])
                c0 = _counters(lib)
                rc, inner = do_gemms(len(out), kind, blocks, gs)
                e = dict(call=kind, rc=rc, inner=inner)
                e.update({k: b - a for k, a, b in zip(COUNTERS, c0, _counters(lib))})
                out.append(e)
    finally:
        lib.pa_gemm_split_config(0, None, 0)
        lib.pa_gemm_split_cache_use(None)
        if sc["cache"]:
            lib.pa_gemm_split_cache_destroy(cache)
    return out


# ------------------------------------------------------------------------------------------------------------------- dry driver
def dry_run(lib, sc, states=None):
    """Replays a scenario through pa_gemm_split_plan(commit = 1): no GPU.  `states`: a dict that receives, per entry index of a
    GEMM call, the plan's own fields and the context state it reports, one dict per member - for checks beyond the golden fields."""
    from plankassembly_amd import _lib as L
    nxt = [0x7e0000000000]

    def base_of(name, n):
        b = nxt[0]
        nxt[0] += (n + 4095) // 4096 * 4096 + 4096
        return b

    sp = _Space(sc, base_of)

    def plan(k, kind, blocks, gs):
        n = len(blocks)
        info = (L.SplitPlanInfo * n)()
        rc = lib.pa_gemm_split_plan(blocks, n, 1, info)
        assert rc == 0, rc
        if states is not None:
            states[k] = [info_dict(L, info[i]) for i in range(n)]
        if kind == "group" and not info[0].taken:
            return -1, []                                      # (pa_gemm_group answers PA_EINVAL and records nothing)
        inner = [dry_block(L, sp, blocks[i], info[i]) for i in range(n)]
        # the status of a pa_gemm call is its inner call's: the dispatch's own dry run (pa_gemm_plan) over the planned block
        return (inner_status(lib, L, sp, blocks[0], info[0]) if kind == "gemm" else 0), inner

    return _run(lib, L, sc, sp, sp.base.get("cache"), plan)


def info_dict(L, o):
    return dict(taken=o.taken, pat=o.pat, drop_seg=o.drop_seg, drop_fwd=o.drop_fwd,
                source=[L.SPLIT_SRC[s] for s in o.source], mode=list(o.mode), blocks=list(o.blocks), off=list(o.off),
                bytes=list(o.bytes), keep_off=o.keep_off, long_off=o.long_off, nkeep=o.nkeep, nkeepL=o.nkeepL,
                long_closed=o.long_closed)


def inner_status(lib, L, sp, a, o):
    b = L.GemmArgs.from_buffer_copy(a)
    b.M, b.N, b.K, b.lda, b.ldb, b.sA, b.sB, b.splitk = o.M, o.N, o.K, o.lda, o.ldb, o.sA, o.sB, o.splitk
    if o.taken:
        at = [sp.base["cache" if L.SPLIT_SRC[s].startswith("cache") else "scratch"] + off for s, off in zip(o.source, o.off)]
        b.in_dtype, b.A, b.B = L.PA_BF16, at[0], at[1]
        if a.aux:
            b.aux, b.ldaux, b.sAux = at[2], o.N, o.M * o.N
    return lib.pa_gemm_plan(C.byref(b), None, C.byref(L.GemmPlanInfo()))


def dry_block(L, sp, a, o):
    """The inner argument block a plan entry stands for, in the golden file's form."""
    def operand(k, own):
        src = L.SPLIT_SRC[o.source[k]]
        if src == "caller":
            return sp.where(own)
        return ["cache" if src.startswith("cache") else "scratch", o.off[k]]
    return dict(A=operand(0, a.A), B=operand(1, a.B), aux=operand(2, a.aux), M=o.M, N=o.N, K=o.K, lda=o.lda, ldb=o.ldb,
                sA=o.sA, sB=o.sB, splitk=o.splitk, splitk_defer=a.splitk_defer)


# ------------------------------------------------------------------------------------------------------------------- real driver
def real_run(lib, sc, errors=None, dry_check=False, seed=0):
    """Runs a scenario on cuda:0.  `errors`: a list that receives (entry index, member, taken, error) for every GEMM output, the
    error being max |got - ref| / max (|a| |b|) against the float64 product.  dry_check: before each GEMM call the dry run
    (commit = 0) over the same addresses must give the blocks the real call then records."""
    import torch
    from plankassembly_amd import _lib as L
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(seed)
    tens = {}

    def base_of(name, n):
        if name in ("scratch", "cache"):
            t = torch.zeros(n + 256, dtype=torch.uint8, device=dev)
            tens[name] = t
            return (t.data_ptr() + 255) // 256 * 256
        t = torch.randn(n // 4 + 64, generator=gen).to(dev)     # (64 spare floats: operands that start a few bytes in)
        tens[name] = t
        assert t.data_ptr() % 256 == 0
        return t.data_ptr()

    sp = _Space(sc, base_of)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def wrote(ptr, src, rows, cols, ld, pat):
        # the producer's side of pa_gemm_split_reserve: write the cut image of src
        name, off = (src, 0) if isinstance(src, str) else src
        x = torch.as_strided(tens[name], (rows, cols), (ld, 1), off // 4)
        hi = x.to(torch.bfloat16)
        lo = (x - hi.float()).to(torch.bfloat16)
        o = ptr - tens["scratch"].data_ptr()
        img = tens["scratch"][o: o + rows * cols * 6].view(torch.bfloat16).view(rows, 3 * cols)
        img.copy_(torch.cat([hi, hi, lo] if pat == 0 else [hi, lo, hi], dim=1))

    def run(k, kind, blocks, gs):
        n = len(blocks)
        want = None
        if dry_check:
            info = (L.SplitPlanInfo * n)()
            assert lib.pa_gemm_split_plan(blocks, n, 0, info) == 0
            want = [dry_block(L, sp, blocks[i], info[i]) for i in range(n)] if (kind == "gemm" or info[0].taken) else []
        sks = [lib.pa_gemm_effective_splitk(g["K"], PA_F32, g.get("splitk", 1)) for g in gs]      # (slabs, in this mode's tiling)
        out2 = (C.c_int64 * 2)()
        lib.pa_gemm_split_stats(out2, 0)
        lib.pa_gemm_record(1)
        rc = lib.pa_gemm(blocks, stream) if kind == "gemm" else lib.pa_gemm_group(blocks, n, stream)
        cnt = lib.pa_gemm_record(0)
        rec = (L.GemmArgs * max(cnt, 1))()
        cnt = lib.pa_gemm_recorded(rec, cnt)
        inner = [_block(sp, rec[i]) for i in range(cnt)]
        if want is not None:
            assert want == inner, (gs, want, inner)
        if errors is not None and rc == 0:
            out3 = (C.c_int64 * 2)()
            lib.pa_gemm_split_stats(out3, 0)
            torch.cuda.synchronize()
            for i, g in enumerate(gs):
                errors.append((k, i, out3[0] > out2[0], _error(torch, tens, g, sks[i])))
        return rc, inner

    out = _run(lib, L, sc, sp, sp.base.get("cache"), run, wrote)
    torch.cuda.synchronize()
    return out


def _error(torch, tens, g, slabs):
    """max |got - ref| / max (|a| |b|) of one GEMM call against the float64 product of its operands as they lie in the buffers."""
    M, N, K, nb = g["M"], g["N"], g["K"], g.get("batch", 1)

    def mat(ref, rows, cols, ld, stride, b):
        name, off = ref
        return torch.as_strided(tens[name], (rows, cols), (ld, 1), off // 4 + b * stride).cpu().double()
    worst = 0.0
    for b in range(nb):
        sA, sB = g.get("sA", M * K if nb > 1 else 0), g.get("sB", N * K if nb > 1 else 0)
        lda, ldb = g.get("lda", K if g["akc"] else M), g.get("ldb", K if g["bkc"] else N)
        a = mat(g["A"], M, K, lda, sA, b) if g["akc"] else mat(g["A"], K, M, lda, sA, b).t()
        bm = mat(g["B"], N, K, ldb, sB, b).t() if g["bkc"] else mat(g["B"], K, N, ldb, sB, b)
        ref, bound = a @ bm, float((a.abs() @ bm.abs()).max())
        if g.get("aux"):
            gate = mat(g["aux"], M, N, N, M * N, b)
            ref = torch.where(gate > 0, ref * g.get("aux_scale", 1.0), torch.zeros_like(ref))
        if g.get("defer"):
            got = torch.as_strided(tens[g["ws"][0]], (slabs, M, N), (M * N, N, 1), g["ws"][1] // 4).cpu().double().sum(0)
        else:
            got = mat(g["C"], M, N, N, M * N, b)
        worst = max(worst, float((got - ref).abs().max()) / bound)
    return worst


def write_golden(golden):
    """One call per line."""
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(
            json.dumps(name) + ":[\n" + ",\n".join(json.dumps(e, sort_keys=True, separators=(",", ":")) for e in golden[name]) + "\n]"
            for name in sorted(golden)) + "\n}\n")


def record():
    lib = load_lib(dry=False)
    S = scenarios()
    golden = {name: real_run(lib, sc) for name, sc in S.items()}
    write_golden(golden)
    n = sum(len(v) for v in golden.values())
    print(f"recorded {len(golden)} scenarios, {n} calls -> {GOLDEN}")


if __name__ == "__main__":
    if "--record" in sys.argv:
        record()
    else:
        sys.exit("usage: PLANK_HIP_LIB=<library of the parent commit> python tests/x3_plan_scenarios.py --record")
