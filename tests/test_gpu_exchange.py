"""The two exchange buffers of a staged evaluation (eval_pass1 / eval_pass2 / eval_finish on caller-owned device buffers),
entry by entry, on every kernel family that fills them: small.hip, mid.hip with one tile, mid.hip with two tiles and its Gram
launch pair or the engine's launch, and the engine's row chunks.  The reference and its bound are tests/exchange_ref.py (80
bits, from the device's own U^-1, r, 1/s, v, w and X of the same evaluation); conditions on the reference alone are checked in
tests/test_exchange_host.py, which runs over the case list of this module.  fp64 problems only (fp32-bulk problems store V in
float and need another bound); batch lanes, RCCL contexts and eval_targets are pinned elsewhere.

Cases are tests/util.py::factor_case (cond(K_m + jitter I) <= 1e5), sigma2 = 0.1; the path is asserted from last_timings().
Chunked cases (chunk_rows given) have no "x_rows", so their column block and E scalars are checked for padding and for being
written, not against the reference.  Figures: profiles/exchange_margins.txt (GPR_MARGINS_LOG, tests/margins.py).

What the checks found: Cov_se_fat WITHOUT a projection on small.hip and mid.hip left the D x d `Proj block of exchange 2
unwritten (the reductions sized it by the kernel's D, zero without a projection): check 3 at fat_ms and fat_het on small,
fat_het on mid with one and with two tiles.
"""
import collections
import functools

import numpy as np
import pytest

import gpr_amd
from gpr_amd import _lib
from tests import exchange_ref as R
from tests import margins as M
from tests.test_gpu_parity import TOL_SHARD, TOL_SHARD_GRAD
from tests.util import factor_case, taken

gpu = pytest.mark.gpu
SIGMA2, SIGMA2_NEXT, SENTINEL = 0.1, 0.37, 1e300

Case = collections.namedtuple("Case", "path kind n m d D chunk variational model_only log_sf2 env",
                              defaults=(None, 0, False, False, 0.0, ()))
ENGINE = (("GPRHIP_SMALL_PATH", "0"), ("GPRHIP_MID_PATH", "0"))
NO_GRAM = (("GPRHIP_MID_GRAM", "0"),)


def _cases():
    out = []

    def add(path, kind, n, m, d=None, **kw):
        d = (2 if kind == "iso" else 3) if d is None else d
        c = Case(path, kind, n, m, d, **kw)
        if c not in out:
            out.append(c)

    for m in (1, 17, 64):                      # small.hip: 64-row blocks
        for n in (1, 63, 64, 65, 200):
            add("small", "iso", n, m)
    for d in (1, 3, 16):
        add("small", "iso", 200, 17, d)
    add("small", "iso", 64 * 512 + 65, 17)     # a workgroup takes more than one block
    for m in (65, 128):                        # mid.hip, one tile
        add("mid1", "iso", 200, m)
    add("mid1", "iso", 64 * 256 + 65, 65)
    for m in (129, 256):                       # mid.hip, two tiles: three packed tiles
        add("mid2", "iso", 200, m)
    for n in (4096, 4097, 32 * 256 + 33):      # MID_GRAM_ROWS: own launch pair / the engine's launch (smallest m: n m^2 in 80 bits)
        add("mid2", "iso", n, 129)
    add("mid2", "iso", 200, 129, env=NO_GRAM)
    for m in (257, 385):                       # engine: 6 and 10 packed tiles, ragged last chunk
        add("engine", "iso", 300, m, chunk=128)
        add("engine", "iso", 700, m, chunk=256)
    add("engine", "iso", 300, 385)             # one chunk: the column block and the E scalars at mp = 512 have a reference
    for m in (17, 129):
        add("engine", "iso", 300, m, env=ENGINE)
    for path, m, env in (("small", 17, ()), ("mid2", 129, ()), ("engine", 17, ENGINE)):   # Cov_se_fat: D 5, d 3
        add(path, "fat_proj_het", 200, m, 3, D=5, env=env)
    for path, env in (("small", ()), ("engine", ENGINE)):
        add(path, "fat_ms", 200, 17, 3, env=env)
    # Cov_se_fat with neither a projection nor multiscales: the layout keeps its D x d `Proj block, which no kernel fills
    for path, m, env in (("small", 17, ()), ("mid1", 65, ()), ("mid2", 129, ()), ("engine", 17, ENGINE)):
        add(path, "fat_het", 200, m, 3, env=env)
    for path, n, m, kw in (("small", 200, 17, {}), ("mid1", 200, 65, {}), ("mid2", 200, 129, {}),
                           ("engine", 300, 257, dict(chunk=128))):
        add(path, "iso", n, m, variational=True, **kw)
        add(path, "iso", n, m, model_only=True, **kw)
        add(path, "iso", n, m, log_sf2=0.3, **kw)
    return out


def case_id(c):
    s = "%s-%s-n%d-m%d-d%d" % (c.path, c.kind, c.n, c.m, c.d)
    s += ("-c%d" % c.chunk if c.chunk else "") + ("-var" if c.variational else "") + ("-model" if c.model_only else "")
    s += ("-sf2" if c.log_sf2 else "") + "".join("-" + k[7:].lower() + v for k, v in c.env)
    return s


CASES = _cases()
# one case per path for the checks that do not need every shape
PER_PATH = {"small": Case("small", "iso", 200, 17, 2), "mid1": Case("mid1", "iso", 200, 65, 2),
            "mid2": Case("mid2", "iso", 200, 129, 2), "engine": Case("engine", "iso", 300, 257, 2, chunk=128)}


@functools.lru_cache(maxsize=None)
def data(kind, n, m, d, D):
    return factor_case(kind, n, m, d, D)


def hypers(c):
    """(X, y, Z, keyword arguments of eval_pass1 / eval, keyword arguments of exchange_ref.reference)"""
    X, y, Z, args, ok, cond = data(c.kind, c.n, c.m, c.d, c.D)
    args = dict(args, log_sf2=c.log_sf2)
    hyp = dict(sigma2=SIGMA2, inducing=Z, variational=c.variational, model_only=c.model_only, **args)
    ref = dict(iso=c.kind == "iso", log_sf2=c.log_sf2, sigma2=SIGMA2, log_ell=args.get("log_ell", 0.0), tproj=args.get("tproj"),
               log_ms=args.get("log_multiscales_m05"), variational=c.variational)
    return X, y, Z, hyp, ref


@functools.lru_cache(maxsize=None)
def layout_of(fat, D, d, m):
    lib = _lib.load()
    return R.layout(lib.gprhip_exchange_len, lib.gprhip_exchange_offset, fat, D, d, m)


def layout_for(c, X):
    return layout_of(c.kind != "iso", X.shape[0], c.d, c.m)


def path_of(stages, mp):
    t = taken(stages)
    return t if t != "mid" else ("mid1" if mp == 128 else "mid2")


# ---- the GPU half -----------------------------------------------------------------------------------------------------------
def _problem(c, X, y, monkeypatch, env=None, chunk=None):
    for k in ("GPRHIP_SMALL_PATH", "GPRHIP_MID_PATH", "GPRHIP_MID_GRAM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (c.env if env is None else env):
        monkeypatch.setenv(k, v)          # read when the problem is created
    p = gpr_amd.Problem(gpr_amd.COV_SE_ISO if c.kind == "iso" else gpr_amd.COV_SE_FAT, X.shape[1], X.shape[0], c.d, c.m,
                        chunk_rows=c.chunk if chunk is None else chunk)
    p.set_inputs(X)
    p.set_targets(y)
    p.set_timing(2)
    return p


def _buf(length, fill):
    import torch
    t = torch.full((length,), fill, dtype=torch.float64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()      # (the library works on a stream of its own)
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def _staged(p, hyp, n_total, fill=0.0, want_grad=True, spoil=None):
    """One staged evaluation of a single problem on buffers pre-filled with `fill`: (exchange 1, exchange 2, Evaluation).
    spoil(lay-less callable on the torch buffer), if given, is applied to exchange 1 before pass 2 and to exchange 2 before the
    finish stage."""
    a1, a2 = _buf(p.ar1_len(), fill), _buf(p.ar2_len(), fill)
    p.eval_pass1(a1.data_ptr(), n_total, want_grad=want_grad, **hyp)
    p.sync()
    b1 = _host(a1)
    if spoil is not None:
        spoil(a1)
    p.eval_pass2(a1.data_ptr(), a2.data_ptr())
    p.sync()
    b2 = _host(a2)
    if spoil is not None:
        spoil(a2)
    ev = p.eval_finish(a2.data_ptr())
    return b1, b2, ev


def _ops(p, X, y, Z, model_only, with_x):
    n = X.shape[1]
    return dict(inputs=X, Z=Z, y=None if model_only else y, uinv=p.debug_fetch_matrix("uinv"), r=p.debug_fetch("r"),
                is_=p.debug_fetch("is"), v=p.debug_fetch("v"), w=p.debug_fetch("w"),
                X=p.debug_fetch_matrix("x_rows", n) if with_x else None)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def _same_eval(a, b):
    ok = all(_same_bits(getattr(a, k), getattr(b, k)) for k in ("l1", "l2", "l", "coeffs"))
    if a.grad is not None or b.grad is not None:
        ok = ok and _same_bits(a.grad, b.grad) and _same_bits(a.dl_dsigma2, b.dl_dsigma2)
    return ok


class _Bad(list):
    def check(self, ok, what):
        if not ok:
            self.append(what)

    def done(self, label):
        assert not self, "%s: %s" % (label, "; ".join(self))


def check_reference(bad, b1, b2, ref, prefix=""):
    """Check 1: every entry with a reference within its bound; every ratio recorded."""
    for which, got in ((1, b1), (2, b2)):
        rat = R.ratios(got, ref["ref%d" % which], ref["bound%d" % which], ref["has%d" % which], ref["cls%d" % which])
        for name, (worst, pos) in rat.items():
            M._record("%sex%d_%s" % (prefix, which, name), worst, 1.0, pos=pos)
            bad.check(worst <= 1.0, "%sexchange %d, %s: %.3g x its bound at position %d (got %r, reference %r)" % (
                prefix, which, name, worst, pos, float(got[pos]), float(ref["ref%d" % which][pos])))


def check_padding(bad, b1, b2, ref):
    """Check 2: padded entries and unused tail slots are +0.0 bit for bit; entries below the diagonal are finite."""
    for which, got in ((1, b1), (2, b2)):
        cls = ref["cls%d" % which]
        zero = np.isin(cls, [R._CLS["pad"], R._CLS["unused"]])
        wrong = zero & ((got != 0.0) | np.signbit(got))
        bad.check(not wrong.any(), "exchange %d: %d padded or unused entries are not +0.0, the first at position %d (%r)" % (
            which, int(wrong.sum()), int(np.argmax(wrong)), float(got[int(np.argmax(wrong))])))
        bad.check(bool(np.all(np.isfinite(got))), "exchange %d holds a non-finite entry" % which)


def full_check(c, p, X, y, Z, hyp, refkw, n_total, label, prefix=""):
    """Checks 1-3 of one problem and one set of hyper-parameters (after a gradient evaluation)."""
    bad = _Bad()
    z1, z2, ev0 = _staged(p, hyp, n_total, 0.0)
    s1, s2, ev1 = _staged(p, hyp, n_total, SENTINEL)
    for which, a, b in ((1, z1, s1), (2, z2, s2)):       # check 3
        diff = a.view(np.int64) != b.view(np.int64)
        bad.check(not diff.any(), "exchange %d: %d entries depend on what the buffer held before, the first at position %d "
                  "(%r after zeros, %r after the sentinel)" % (which, int(diff.sum()), int(np.argmax(diff)),
                                                                float(a[int(np.argmax(diff))]), float(b[int(np.argmax(diff))])))
    bad.check(_same_eval(ev0, ev1), "the finish stage's outputs depend on what the buffers held before")
    lay = layout_for(c, X)
    ref = R.reference(lay, _ops(p, X, y, Z, c.model_only, not c.chunk or X.shape[1] <= c.chunk), **refkw)
    check_reference(bad, z1, z2, ref, prefix)
    check_padding(bad, z1, z2, ref)
    bad.done(label)
    return z1, z2, ev0, ref


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_entry_of_both_buffers(c, monkeypatch):
    """Checks 1, 2, 3"""
    X, y, Z, hyp, refkw = hypers(c)
    M.note(path=c.path, case=case_id(c))
    p = _problem(c, X, y, monkeypatch)
    try:
        full_check(c, p, X, y, Z, hyp, refkw, c.n, case_id(c))
        assert path_of(set(p.last_timings()), layout_for(c, X)["mp"]) == c.path, p.last_timings()
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("name", sorted(PER_PATH))
def test_an_evidence_only_evaluation_touches_the_tail_of_exchange_2_alone(name, monkeypatch):
    """Check 3, second half (the comment at do_pass2): the tail is zeroed, the rest is left as it was, and the finish stage
    returns the same bits from a sentinel-filled buffer as from a zero-filled one."""
    c = PER_PATH[name]
    X, y, Z, hyp, refkw = hypers(c)
    p = _problem(c, X, y, monkeypatch)
    try:
        lay = layout_for(c, X)
        z1, z2, ev0 = _staged(p, hyp, c.n, 0.0, want_grad=False)
        s1, s2, ev1 = _staged(p, hyp, c.n, SENTINEL, want_grad=False)
        assert _same_bits(z1, s1), "exchange 1 depends on what the buffer held before"
        t2 = lay["tail2"]
        assert np.all(z2 == 0.0) and np.all(s2[t2:] == 0.0) and not np.signbit(s2[t2:]).any()
        assert np.all(s2[:t2] == SENTINEL), "an evidence-only pass 2 wrote in front of the tail of exchange 2"
        assert ev0.grad is None and _same_eval(ev0, ev1)
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("name", sorted(PER_PATH))
def test_nothing_reads_below_the_diagonal(name, monkeypatch):
    """Check 4: the entries r > c of the diagonal tiles are finite (check 2 of every case), and overwriting them with the
    sentinel in the reduced buffers -- exchange 1 before pass 2, exchange 2 before the finish stage -- changes no output."""
    c = PER_PATH[name]
    X, y, Z, hyp, refkw = hypers(c)
    lay = layout_for(c, X)
    import torch
    off, m = lay["off"], c.m
    rr, cc = np.nonzero(off >= 0)
    below = torch.as_tensor(off[rr, cc][rr > cc], device=torch.device("cuda", 0))
    assert below.numel() == sum(min(128, lay["mp"] - 128 * t) * (min(128, lay["mp"] - 128 * t) - 1) // 2 for t in range(lay["mp"] // 128))

    def spoil(buf):
        buf[below] = SENTINEL
        torch.cuda.synchronize()

    p = _problem(c, X, y, monkeypatch)
    try:
        _, _, ev0 = _staged(p, hyp, c.n)
        _, _, ev1 = _staged(p, hyp, c.n, spoil=spoil)
        assert _same_eval(ev0, ev1), "an output of the finish stage depends on entries below the diagonal of a diagonal tile"
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("name", sorted(PER_PATH))
def test_a_reweighted_staged_evaluation(name, monkeypatch):
    """Check 7: reuse_v=True with a new sigma2 after a fresh evaluation: checks 1-3 again -- B~, c~ and both tails are those
    of the new 1/s (the reference is formed from the rows fetched after the re-weighted evaluation and the new sigma2)."""
    c = PER_PATH[name]
    X, y, Z, hyp, refkw = hypers(c)
    M.note(path=c.path, case=case_id(c) + "-reuse")
    p = _problem(c, X, y, monkeypatch)
    try:
        z1, _, _ = _staged(p, hyp, c.n)
        r0 = p.debug_fetch("r")
        hyp2 = dict(hyp, sigma2=SIGMA2_NEXT, reuse_v=True)
        w1, _, _, ref = full_check(c, p, X, y, Z, hyp2, dict(refkw, sigma2=SIGMA2_NEXT), c.n, case_id(c) + "-reuse", "reuse_")
        assert np.array_equal(p.debug_fetch("r"), r0), "r changed under reuse_v"
        t1 = layout_for(c, X)["tail1"]
        assert w1[t1] != z1[t1] and not _same_bits(w1[:t1], z1[:t1]), "exchange 1 is still that of the first sigma2"
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("name", sorted(PER_PATH))
def test_call_order(name, monkeypatch):
    """Check 8: pass 2 before pass 1 and the finish stage before pass 2 are refused with ESTATE, and the complete staged
    evaluation that follows is bit-identical to one on a fresh problem."""
    c = PER_PATH[name]
    X, y, Z, hyp, refkw = hypers(c)
    fresh = _problem(c, X, y, monkeypatch)
    p = _problem(c, X, y, monkeypatch)
    try:
        f1, f2, fev = _staged(fresh, hyp, c.n)
        a1, a2 = _buf(p.ar1_len(), 0.0), _buf(p.ar2_len(), 0.0)
        with pytest.raises(gpr_amd.GprHipError) as e:
            p.eval_pass2(a1.data_ptr(), a2.data_ptr())
        assert e.value.status == _lib.ESTATE
        p.eval_pass1(a1.data_ptr(), c.n, **hyp)
        with pytest.raises(gpr_amd.GprHipError) as e:
            p.eval_finish(a2.data_ptr())
        assert e.value.status == _lib.ESTATE
        b1, b2, ev = _staged(p, hyp, c.n)
        assert _same_bits(b1, f1) and _same_bits(b2, f2) and _same_eval(ev, fev)
    finally:
        p.close()
        fresh.close()


def _sharded(c, cuts, envs, monkeypatch, label, mixed=False):
    """Checks 1, 2 and 5 for the row shards [cuts[i], cuts[i+1]) of case c, shard i created under envs[i]: the stage sets of
    the shards, for the caller to compare.
    The sums.  Exchange 1 does not depend on the other shards, so with one family (not `mixed`) its sum is held against the
    reference of the WHOLE problem, formed from the whole problem's own fetched U^-1, r and 1/s (asserted bit-identical to
    every shard's U^-1) within that reference's bound: gamma_L of n terms in any order covers the partition into shards and the
    caller's addition.  Exchange 2 is a function of the summed exchange 1 through v, w and X, which the whole problem
    holds with other roundings than the shards; its sum, and both sums of mixed families (each keeps its own U^-1), are held
    against the shards' references added in 80 bits, which pins the caller's addition and nothing more."""
    import torch
    X, y, Z, hyp, refkw = hypers(c)
    lay = layout_for(c, X)
    whole = _problem(c, X, y, monkeypatch, env=(), chunk=0)
    shards = [_problem(c, np.asfortranarray(X[:, lo:hi]), y[lo:hi].copy(), monkeypatch, env=env, chunk=0)
              for lo, hi, env in zip(cuts[:-1], cuts[1:], envs)]
    try:
        want = whole.eval(**hyp)
        ar1 = [_buf(p.ar1_len(), SENTINEL) for p in shards]
        ar2 = [_buf(p.ar2_len(), SENTINEL) for p in shards]
        for p, a in zip(shards, ar1):
            p.eval_pass1(a.data_ptr(), c.n, **hyp)
            p.sync()
        tot1 = torch.stack(ar1).sum(0)
        torch.cuda.synchronize()
        for p, a in zip(shards, ar2):
            p.eval_pass2(tot1.data_ptr(), a.data_ptr())
            p.sync()
        tot2 = torch.stack(ar2).sum(0)
        torch.cuda.synchronize()
        evs = [p.eval_finish(tot2.data_ptr()) for p in shards]
        bad = _Bad()
        refs = []
        for i, (p, lo, hi) in enumerate(zip(shards, cuts[:-1], cuts[1:])):
            ref = R.reference(lay, _ops(p, np.asfortranarray(X[:, lo:hi]), y[lo:hi], Z, c.model_only, True), **refkw)
            b1, b2 = _host(ar1[i]), _host(ar2[i])
            check_reference(bad, b1, b2, ref, "shard_")
            check_padding(bad, b1, b2, ref)
            refs.append(ref)
        # the sum: the shards' references added in 80 bits (the reference of the whole problem when the shards hold the same
        # U^-1 bit for bit; with mixed families each keeps its own), within the sum of their bounds and the k - 1 roundings of
        # the sum itself
        k = len(shards)
        total = {}
        for which, tot in ((1, tot1), (2, tot2)):
            key = "ref%d" % which
            total[key] = sum(r[key] for r in refs)
            total["bound%d" % which] = sum(r["bound%d" % which] for r in refs) + \
                (k - 1) * R.U * np.asarray(sum(np.abs(r[key]) for r in refs), np.float64)
            total["has%d" % which], total["cls%d" % which] = refs[0]["has%d" % which], refs[0]["cls%d" % which]
        check_reference(bad, _host(tot1), _host(tot2), total, "sum_")
        if not mixed:
            ui = whole.debug_fetch_matrix("uinv")
            bad.check(all(_same_bits(ui, p.debug_fetch_matrix("uinv")) for p in shards), "the shards' U^-1 is not the whole problem's")
            wref = R.reference(lay, dict(inputs=X, Z=Z, y=None if c.model_only else y, uinv=ui, r=whole.debug_fetch("r"),
                                         is_=whole.debug_fetch("is"), v=None), **refkw)
            got = _host(tot1)
            for name, (worst, pos) in R.ratios(got, wref["ref1"], wref["bound1"], wref["has1"], wref["cls1"]).items():
                M._record("whole_ex1_" + name, worst, 1.0, pos=pos)
                bad.check(worst <= 1.0, "summed exchange 1 against the whole problem's reference, %s: %.3g x its bound at %d" % (name, worst, pos))
        fams = M.families("iso", c.d, c.m)
        for ev in evs:
            M.check_rel("l", ev.l, want.l, TOL_SHARD)
            M.check_rel("dl_dsigma2", ev.dl_dsigma2, want.dl_dsigma2, TOL_SHARD)
            M.check_grad(ev.grad, want.grad, fams, TOL_SHARD_GRAD)
            M.check_vec("coeffs", ev.coeffs, want.coeffs, TOL_SHARD_GRAD)
        bad.done(label)
        return [frozenset(p.last_timings()) for p in shards]
    finally:
        for p in shards + [whole]:
            p.close()


@gpu
@pytest.mark.parametrize("nshards", [2, 3])
@pytest.mark.parametrize("name", sorted(PER_PATH))
def test_ragged_shards(name, nshards, monkeypatch):
    """Check 5: 2 and 3 ragged shards (cut points no multiples of 64) of one case per path"""
    c = PER_PATH[name]._replace(n=700, chunk=0)
    cuts = (0, 333, 700) if nshards == 2 else (0, 205, 466, 700)
    M.note(path=c.path, case="%s-shards%d" % (case_id(c), nshards))
    stages = _sharded(c, cuts, [c.env] * nshards, monkeypatch, "%s, %d shards" % (case_id(c), nshards))
    assert all(path_of(s, layout_of(False, c.d, c.d, c.m)["mp"]) == c.path for s in stages), stages


@gpu
def test_three_families_in_one_sum_at_two_tiles(monkeypatch):
    """Check 6: m = 129, n = 400: the engine, mid.hip with the engine's Gram launch, and mid.hip with its own launch pair"""
    c = Case("mixed", "iso", 400, 129, 2)
    M.note(path="mixed", case="mixed-m129")
    stages = _sharded(c, (0, 131, 277, 400), [ENGINE, NO_GRAM, ()], monkeypatch, "mixed m = 129", mixed=True)
    # last_timings() tells the engine's shard from the two of mid.hip, but both Gram launches of mid.hip run under the one stage
    # name p1_syrk_B / p2_syrk_W (gram_over_v).  That GPRHIP_MID_GRAM=0 took effect shows in the bits: on the rows of the second
    # shard the switched problem and a plain one fill the tiles of exchange 1 in another order of additions -- both within the
    # bound (the shard above, and every mid2 case), not bit for bit the same; everything behind the tiles but c~ comes from the
    # one row kernel and is
    assert [taken(s) for s in stages] == ["engine", "mid", "mid"] and stages[0] != stages[1], stages
    X, y, Z, hyp, refkw = hypers(c)
    lay = layout_for(c, X)
    got = []
    for env in (NO_GRAM, ()):
        p = _problem(c, np.asfortranarray(X[:, 131:277]), y[131:277].copy(), monkeypatch, env=env, chunk=0)
        try:
            got.append(_staged(p, hyp, c.n)[0])
        finally:
            p.close()
    assert not _same_bits(got[0][:lay["packed"]], got[1][:lay["packed"]]), "GPRHIP_MID_GRAM=0 changed nothing in the tiles"
    assert _same_bits(got[0][lay["tail1"]:], got[1][lay["tail1"]:])


@gpu
def test_two_families_in_one_sum_at_few_inducing_points(monkeypatch):
    """Check 6: m = 17: small.hip and the engine"""
    c = Case("mixed", "iso", 400, 17, 2)
    M.note(path="mixed", case="mixed-m17")
    stages = _sharded(c, (0, 131, 400), [(), ENGINE], monkeypatch, "mixed m = 17", mixed=True)
    assert [taken(s) for s in stages] == ["small", "engine"], stages
