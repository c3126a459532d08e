"""Every entry of the gradient of the log evidence against tests/hyper_grad_ref.py: the 80-bit contraction of the analytic
covariance derivatives with the DEVICE'S OWN W, X and v of the same evaluation (debug_fetch), within the derived running-error
bound (L + C) u A[theta] of that module.  The factors and row operands are pinned elsewhere (tests/test_gpu_factors.py,
tests/test_gpu_row_operands.py); here conditioning never enters, no oracle and no Problem.condition() are used, and what is
under test is the last stage alone: the gradient kernels, the K_m trace kernels, the reductions between them and the host's
assembly.  tests/test_hyper_grad_host.py pins the reference and the bound on the CPU over the same list of cases.

Case -> kernel, read off the dispatch code (grad_mfma.hip:301-333, rowops.hip:580-615, finalize.hip:302-343,
gprhip.hip:1353-1398); all fp64, one row chunk unless stated:
  engine, m = 257 (three column blocks, one live column in the last; m = 50, 129 with the one-kernel paths switched off)
    iso d = 3, 4 | 5, 8 | 9, 16 | 17, 32 | 33, 64     grad_mfma_kernel<1,1,0> | <2,1,0> | <4,1,0> | <8,2,0> (all PF) | <16,4,0>;
                                                      km_traces_kernel<4 | 8 | 16 | 32 | 64>
    proj (D, d) = (16,3) (17,5) (32,9) (33,17)        <1,1,1> <2,1,2> <4,1,2> (PF) <8,2,4> (single buffer), each with K resident
                  (64,33) (40,40)                     <16,4,4> <16,4,4>            (KR) and with GPRHIP_K_RESIDENT=0;
                                                      proj_inducing_grad_kernel, proj_term2_kernel
    n = 1 .. 200, GPRHIP_GRAD_SLAB = 64, 128          ragged 16-row tiles, 64-row chunks and slabs of <1,1,0>
    m = 385, 641, 1100                                4, 6, 9 column blocks; km_slab_rows 8 -> 32 at m = 1100
    GPRHIP_GRAD_SCALAR=1, d x D                       grad_fused_kernel<4 | 8 | 16 | 32 | 64, 0 | 8 | 32 | 64>
    multiscales d = 3                                 grad_fused_ms_kernel<4,0>, km_traces_ms_kernel<4>
    d = 65; D = 65                                    grad_wide_kernel, km_traces_wide_kernel (d = 65)
  small (m <= 64)  pass 2 and the finish of small.hip;  mid (65 <= m <= 256)  those of mid.hip, one and two tiles, the Gram
    launch pair up to 4096 rows and the engine's launch above.
  offsets 1e3, 1e5 in every coordinate; variational and model_only once per path; (n, m) = (700, 257), (700, 65) in three
    row chunks against the single-chunk gradient within 2 (L + C) u A of the single-chunk operands (X of a chunked
    evaluation cannot be fetched).
Offsets on the small path: 1e3 and 3e3, not 1e5.  Pass 2 of small.hip adds the moments sum_r p_kr E_rc against the
coordinates as given (small_pass2_body.inc:190; grad_fused_kernel does the same, rowops.hip:288), so there the bound grows with
the offset itself and not only through the centroid-shifted kappa: at 1e5 A[theta] is 1.6e7 max |g| of the inducing family,
beyond the 1e6 that tests/test_hyper_grad_host.py asks of every case, at 3e3 it is 4.8e5.  This is a known accuracy limit of
that path, not modelled away: the case is the largest offset the headroom admits.
Multiscales with a projection run at D = 8 and 32 (grad_fused_ms_kernel<4, 8 | 32>, launch_reduce_rowes: the row sums
sum_c E_rc / ms_kc are added up from E there, so the Proj family carries no allowance for the row identity).
Left out: the fp32-bulk instantiations (they read a float X that x_rows does not expose).
Cases that add nothing but are the issue's: at n <= 200, m = 257 the library's own slab is 64 rows already (gprhip.hip:699), so
GPRHIP_GRAD_SLAB=64 at n = 63, 64, 65 repeats the default cases bit for bit; the chunked mid case (700, 65) is bit-identical
to its single-chunk run, because pass 2 of mid.hip is one launch over all rows whatever the chunks (gprhip.hip:1220-1231) --
only proj_term2 walks the chunks there; the projected chunked case reaches that loop, and is bit-identical as well, since
its 256-row workgroups coincide with the 256-row chunks (rowops.hip:534).

The Proj family: the second term of its entries, sum_r x_br p_kr es_r, takes es_r = sum_c E_rc not from E but from the row
identity qd - v (sf2 - r) - w sb of pass 2 (rowops.hip:124), whose rounding error has the size of its cancelling terms, not of
E.  Where the projection is square and the covariances are small -- (D, d) = (40, 40), and GPRHIP_GRAD_SCALAR=1 at d = D = 64 --
that error (1.4e-15, 1.7e-15) is 4.6 x and 1.1e7 x the bound of the contraction alone, so the reference models the identity from
the fetched r, 1/s, w and the targets (tests/hyper_grad_ref.py, Proj); with it the worst Proj ratio is 0.002.  In exactly those
cases the allowance is 1e7 to 1e12 times the contraction's own term, so a dropped row or tile would NOT show in their Proj
family: <16,4,4> and the scalar <64,64> are pinned through their inducing and Log_sf2 entries (same E, same accumulators'
column sums), and the Proj accumulation through the cases with larger covariances, (16,3) to (33,17).
"""
import collections
import functools

import numpy as np
import pytest

import gpr_amd
from tests import hyper_grad_ref as H
from tests import margins as M
from tests.util import factor_case
from tests.util import taken as _taken

gpu = pytest.mark.gpu

SIGMA2 = 0.1

Case = collections.namedtuple("Case", "path kind n m d D form env chunk variational model_only offset",
                              defaults=(0, "raw", (), 0, False, False, 0.0))

FORCED = (("GPRHIP_SMALL_PATH", "0"), ("GPRHIP_MID_PATH", "0"))
SCALAR = (("GPRHIP_GRAD_SCALAR", "1"),)
NO_KR = (("GPRHIP_K_RESIDENT", "0"),)


def _cases():
    out = []

    def add(path, kind, n, m, d, D=0, form=None, **kw):
        if form is None:   # how the kernels of the path add the inducing moments (tests/hyper_grad_ref.py)
            form = "shifted_once" if path == "mid" else "shifted" if (path == "engine" and not D and d <= 64 and kind != "fat_ms"
                                                    and SCALAR[0] not in kw.get("env", ())) else "raw"
        c = Case(path, kind, n, m, d, D, form, **kw)
        if c not in out:
            out.append(c)

    # ---- engine, MFMA kernel
    for d in (3, 4, 5, 8, 9, 16, 17, 32, 33, 64):
        add("engine", "iso", 200, 257, d)
    for m in (50, 129):
        add("engine", "iso", 200, m, 3, env=FORCED)
    for D, d in ((16, 3), (17, 5), (32, 9), (33, 17), (64, 33), (40, 40)):
        add("engine", "fat_proj_het", 200, 257, d, D)
        add("engine", "fat_proj_het", 200, 257, d, D, env=NO_KR)
    for n in (1, 15, 16, 17, 63, 64, 65):
        add("engine", "iso", n, 257, 3)
    for slab in (64, 128):
        for n in (slab - 1, slab, slab + 1, 2 * slab + 17):
            add("engine", "iso", n, 257, 3, env=(("GPRHIP_GRAD_SLAB", str(slab)),))
    for m in (385, 641, 1100):
        add("engine", "iso", 300, m, 2)
    # ---- engine, scalar kernels
    for d in (4, 8, 16, 32, 64):
        add("engine", "iso", 200, 257, d, env=SCALAR)
        for D in (8, 32, 64):
            if D >= d:
                add("engine", "fat_proj_het", 200, 257, d, D, env=SCALAR)
    add("engine", "fat_ms", 200, 257, 3)
    for D in (8, 32):
        add("engine", "fat_proj_ms", 200, 257, 3, D)
    add("engine", "iso", 200, 257, 65)
    add("engine", "fat_proj_het", 200, 257, 3, 65)
    # ---- small
    for m in (1, 16, 17, 64):
        add("small", "iso", 200, m, 2)
    for n in (1, 63, 64, 65):
        add("small", "iso", n, 17, 2)
    add("small", "iso", 64 * 512 + 65, 16, 2)
    for d in (1, 8, 9, 16):
        add("small", "iso", 200, 17, d)
    add("small", "fat_het", 200, 17, 3)
    add("small", "fat_proj_het", 200, 17, 3, 16)
    add("small", "fat_proj_het", 200, 17, 5, 17)
    add("small", "fat_ms", 200, 17, 3)
    # ---- mid
    for m in (65, 128):
        for n in (63, 64, 65, 800):
            add("mid", "iso", n, m, 2)
    for m in (129, 256):
        for n in (31, 32, 33, 800, 4096, 4097):
            add("mid", "iso", n, m, 2)
    for m in (65, 129):
        for d in (3, 16):
            add("mid", "iso", 800, m, d)
        add("mid", "fat_proj_het", 800, m, 3, 5)
    # ---- objectives, offsets
    for path, n, m in (("small", 200, 17), ("mid", 800, 65), ("engine", 200, 257)):
        add(path, "iso", n, m, 2, variational=True)
        add(path, "iso", n, m, 2, model_only=True)
        for off in (1e3, 3e3 if path == "small" else 1e5):   # (see the docstring: small.hip's moments are not shifted)
            add(path, "iso", n, m, 3, offset=off)
    for off in (1e3, 1e5):
        add("engine", "iso", 200, 257, 17, offset=off)
    return out


def case_id(c):
    s = "%s%s-n%d-m%d-d%d" % (c.path + "-" if c.path else "", c.kind, c.n, c.m, c.d)
    if c.D:
        s += "-D%d" % c.D
    for k, val in c.env:
        s += "-" + {"GPRHIP_SMALL_PATH": "nosmall", "GPRHIP_MID_PATH": "nomid", "GPRHIP_GRAD_SCALAR": "scalar",
                    "GPRHIP_K_RESIDENT": "nokr", "GPRHIP_GRAD_SLAB": "slab"}[k] + (val if k == "GPRHIP_GRAD_SLAB" else "")
    if c.chunk:
        s += "-c%d" % c.chunk
    if c.offset:
        s += "-off%g" % c.offset
    return s + ("-var" if c.variational else "") + ("-model" if c.model_only else "")


CASES = _cases()
CHUNKED = [Case("engine", "iso", 700, 257, 2, 0, "shifted", chunk=256), Case("mid", "iso", 700, 65, 2, 0, "shifted_once", chunk=256),
           Case("mid", "fat_proj_het", 700, 65, 3, 5, "shifted_once", chunk=256)]


def host_key(c):
    """The case less what the CPU half does not see (path, form, environment, chunks)"""
    return c._replace(env=(), form="raw", chunk=0, path="")


@functools.lru_cache(maxsize=None)
def _factor_case(kind, n, m, d, D):
    return factor_case(kind, n, m, d, D or None)


def data(c):
    """Inputs, targets, inducing points and the hyper-parameter arguments of a case; an offset moves inputs and inducing
    points alike (no projection there), so the covariances stay what they were."""
    X, y, Z, args, ok, cond = _factor_case(c.kind, c.n, c.m, c.d, c.D)
    if c.offset:
        assert "tproj" not in args
        X, Z = np.asfortranarray(X + c.offset), np.asfortranarray(Z + c.offset)
    return X, y, Z, args


def reference_of(c, W, Xr, v, X, Z, args, rows=None):
    return H.reference(W, Xr, v, X, Z, iso=c.kind == "iso", log_sf2=args["log_sf2"], log_ell=args.get("log_ell", 0.0),
                       tproj=args.get("tproj"), log_hetero=args.get("log_hetero_skedasticity"),
                       log_ms=args.get("log_multiscales_m05"), form=c.form, rows=rows)


def check_entries(label, got, ref, factor=1.0, prefix="dev", key=""):
    """Every entry within factor x its bound; the worst ratio of every family is recorded first."""
    assert got.shape == ref["g"].shape, (label, got.shape, ref["g"].shape)
    assert np.all(np.isfinite(got)), label
    rat = H.ratios(got, ref)
    bad = {}
    for (name, sl) in ref["fams"]:
        if name not in rat:
            continue
        r, at = rat[name]
        M.record("%s.%s" % (prefix, name), r / factor, 1.0, case=label, key=key, L=float(ref["L"][sl][0]), C=H.C,
                 scale=float(np.max(np.abs(ref["g"][sl]))), A=float(ref["A"][sl][at]))
        if not r <= factor:
            i = sl.start + at
            bad[name] = "entry %d of the family: got %r, reference %r, bound %.3e (x %.2f)" % (
                at, float(got[i]), float(ref["g"][i]), factor * ref["bound"][i], r / factor)
    assert not bad, (label, bad)


def _cov(kind):
    return gpr_amd.COV_SE_ISO if kind == "iso" else gpr_amd.COV_SE_FAT


def _evaluate(c, monkeypatch, chunk=None):
    """One evaluation: (gradient, W, X rows or None, v, the row vectors behind the Proj family's row identity or None)"""
    for k, val in c.env:
        monkeypatch.setenv(k, val)        # read when the problem is created
    X, y, Z, args = data(c)
    chunk = c.chunk if chunk is None else chunk
    p = gpr_amd.Problem(_cov(c.kind), c.n, X.shape[0], c.d, c.m, chunk_rows=chunk)
    try:
        p.set_inputs(X)
        p.set_targets(y)
        p.set_timing(2)
        ev = p.eval(sigma2=SIGMA2, inducing=Z, variational=c.variational, model_only=c.model_only, **args)
        stages = set(p.last_timings())
        assert _taken(stages) == c.path, (case_id(c), stages)
        W = p.debug_fetch_matrix("w_mat")
        Xr = p.debug_fetch_matrix("x_rows", c.n) if chunk == 0 else None
        rows = None
        if "tproj" in args:
            rows = dict(r=p.debug_fetch("r"), is_=p.debug_fetch("is"), w=p.debug_fetch("w"), y=None if c.model_only else y,
                        variational=c.variational)
        return np.array(ev.grad, dtype=np.float64), W, Xr, p.debug_fetch("v"), rows
    finally:
        p.close()


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_gradient_entry_against_the_80_bit_contraction_of_the_device_operands(c, monkeypatch):
    grad, W, Xr, v, rows = _evaluate(c, monkeypatch)
    X, y, Z, args = data(c)
    check_entries(case_id(c), grad, reference_of(c, W, Xr, v, X, Z, args, rows), key=case_id(host_key(c)))


@gpu
@pytest.mark.parametrize("c", CHUNKED, ids=case_id)
def test_a_chunked_gradient_against_the_single_chunk_one(c, monkeypatch):
    """Three row chunks (256, 256, 188 rows).  X is not kept; the two gradients differ by at most twice the bound of the
    single-chunk operands.  Engine: every product and reduction runs per chunk, the operands differ by rounding.  Mid: pass 2
    is one launch over all rows and the gradient is bit-identical; with a projection proj_term2 runs per chunk, in 256-row
    workgroups that coincide with the chunks, so that one is bit-identical too (profiles/hyper_grad_margins.txt)."""
    one, W, Xr, v, rows = _evaluate(c, monkeypatch, chunk=0)
    X, y, Z, args = data(c)
    ref = reference_of(c, W, Xr, v, X, Z, args, rows)
    check_entries(case_id(c) + "-one", one, ref, key=case_id(host_key(c)))
    many = _evaluate(c, monkeypatch)[0]
    ref_one = dict(ref, g=np.asarray(one, dtype=H.LD))
    check_entries(case_id(c), many, ref_one, factor=2.0, prefix="chunks", key=case_id(host_key(c)))
