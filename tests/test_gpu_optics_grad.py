"""Gradients of the HIP optics step (hd_attenuate_bwd, hd_band_optics_bwd,
hd_band_loop_optics_bwd, hd_rfm_attenuate_bwd through pyharp_amd.opacity and torch autograd)
and of the band epilogue (pyharp_amd.spectral): parity with the float64 torch judge
(tests/optics_grad_ref.py, pinned on the CPU by tests/test_optics_grad_ref.py independently
of the kernels), the bitwise properties of the wave reduction, partial requests, argument
checks, the chain state -> optics -> solver, and CPU tensors.  The judge is the CPU
reference: no finite differences of the GPU against itself, no gradcheck.

Bounds.  The error of a gradient tensor is taken relative to its largest component in the
column.  Against the judge the project's TOL = 1e-6 and, beside it, TIGHT: the same
formulas in the same precision, so what remains is rounding -- ten times the worst error of
the first GPU run (MEASURED, recorded in profiles/optics_grad/parity_margins.json), capped
at 1e-9.
"""

import ctypes
import itertools

import numpy as np
import pytest
import torch

import beer_grad_ref
import optics_grad_ref as ogr
from helpers import TOL, margin
from oracle import harp_np

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CPU = torch.device("cpu")
WB = 32  # kWaveBlock of hd_harp_grad.hip (include/hdharp.h "Summation order")
MEASURED = 1.212e-13  # worst error against optics_grad_ref in the first GPU run (d/dpres of
# the RFM call at 33 waves x 67 columns x 2 layers, 3 species)
TIGHT = min(1.0e-9, 10.0 * MEASURED)
SHAPES = [(1, 1, 1), (WB - 1, 1, 3), (WB, 3, 1), (WB + 1, 67, 2), (2 * WB + 3, 2, 17), (1000, 1, 5)]
EINVAL = 1


def _leaf(x, dev=DEV, grad=True):
    return torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev,
                        requires_grad=grad)


def _col_err(got, ref, col_axis):
    """max |got - ref| over the largest |ref| of the tensor in the column"""
    got, ref = np.asarray(got), np.asarray(ref)
    axes = tuple(i for i in range(ref.ndim) if i != col_axis)
    scale = np.abs(ref).max(axis=axes, keepdims=True)
    return (np.abs(got - ref) / np.maximum(scale, 1e-300)).max()


COL_AXIS = {"conc": 0, "dz": 0, "pres": 0, "temp": 0, "ext0": 1, "x": 1, "bflux": 0, "rho": 0}


def _compare(tag, got, ref):
    worst = 0.0
    for k, g in ref.items():
        assert got[k] is not None, (tag, k)
        assert got[k].shape == g.shape, (tag, k)
        err = _col_err(got[k].cpu().numpy(), g.numpy(), COL_AXIS[k])
        print(f"optics grad {tag} d/d{k}: {err:.3e}")
        worst = max(worst, err)
    return worst


def _both(fn_gpu, fn_ref, inputs, cot_rng):
    """(gpu forward, gpu grads, judge grads) with every input a leaf and one fixed random
    cotangent; the forward under autograd must be bitwise the forward without it"""
    lg = {k: _leaf(v) for k, v in inputs.items()}
    lr = {k: _leaf(v, CPU) for k, v in inputs.items()}
    out = fn_gpu(**lg)
    with torch.no_grad():
        plain = fn_gpu(**{k: v.detach() for k, v in lg.items()})
    assert out.grad_fn is not None and plain.grad_fn is None
    assert torch.equal(out.detach(), plain)
    ref = fn_ref(**lr)
    assert tuple(ref.shape) == tuple(out.shape)
    cot = cot_rng.uniform(-1.0, 1.0, tuple(out.shape))
    out.backward(torch.as_tensor(cot, device=out.device))
    ref.backward(torch.as_tensor(cot))
    fwd = np.abs(out.detach().cpu().numpy() - ref.detach().numpy()).max() / \
        max(np.abs(ref.detach().numpy()).max(), 1e-300)
    assert fwd < 1e-12, fwd
    return out.detach(), {k: v.grad for k, v in lg.items()}, {k: v.grad for k, v in lr.items()}


# ---- table attenuators -------------------------------------------------------------------
class _Tables:
    """three attenuators written as table files: A and B read one species (B with an
    asymmetry table and descending wavelengths), C another (with an asymmetry table)"""

    def __init__(self, tmp, nspecies, const=False):
        from pyharp_amd.opacity import AttenuatorOptions, H2SO4Simple, S8Fuller
        rng = np.random.default_rng(700 + nspecies)
        s1, s2 = (0, 0) if nspecies == 1 else (1, 2)
        self.ref, self.atts = [], []
        for i, (n, sp, g, desc, cls) in enumerate(((5, s1, False, False, S8Fuller),
                                                   (4, s1, True, True, H2SO4Simple),
                                                   (6, s2, True, False, S8Fuller))):
            wl = np.sort(rng.uniform(0.2, 5.0, n))
            if desc:
                wl = wl[::-1].copy()
            kd = np.stack([rng.uniform(0.5, 3.0, n), rng.uniform(0.1, 0.95, n)], axis=1)
            if const:
                kd[:, 0], kd[:, 1] = 2.0, 0.5
            gg = rng.uniform(-0.8, 0.8, n) if g else None
            path = tmp / f"att_{nspecies}_{int(const)}_{i}.txt"
            path.write_text("".join(f"{a!r} {b!r} {c!r}\n" for a, (b, c) in zip(wl.tolist(),
                                                                                  kd.tolist())))
            op = AttenuatorOptions().opacity_files([str(path)]).species_ids([sp]) \
                .species_weights([1.0] * nspecies)
            att = cls(op)
            if g:
                att.set_asymmetry(gg)
            self.atts.append(att)
            self.ref.append((wl, kd, sp, gg))


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("optics_grad")
    return {n: _Tables(tmp, n) for n in (1, 3)}


def _coords(rng, T, nwave):
    """wavelengths inside the tables; then on an inner knot, on the last knot, below and
    above every table, as far as nwave goes"""
    x = rng.uniform(0.3, 4.5, nwave)
    wl = T.ref[0][0]
    for i, v in enumerate((wl[2], wl[-1], 0.05, 9.0, T.ref[1][0][1])):
        if i < nwave:
            x[i] = v
    return x


def _conc(rng, ncol, nlyr, nsp, loop):
    """a species exactly 0 in one layer; a layer without extinction (band_optics) or
    without any scatterer, in the last column, which the other columns' scales never see
    (band_loop_optics: gradients near 1e10 there)"""
    conc = rng.uniform(0.05, 2.0, (ncol, nlyr, nsp))
    if ncol * nlyr > 1 and nsp > 1:  # (with one species that is a layer without scatterer)
        conc[0, nlyr - 1, nsp - 1] = 0.0
    if ncol > 1 or not loop:
        conc[ncol - 1, 0, :] = 0.0
    return conc


@pytest.mark.parametrize("nsp", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_table_attenuators_parity_with_the_judge(shape, nsp, tables):
    from pyharp_amd.opacity import band_loop_optics, band_optics
    nwave, ncol, nlyr = shape
    T = tables[nsp]
    rng = np.random.default_rng(1000 * nwave + 10 * ncol + nsp)
    x = _coords(rng, T, nwave)
    dz = rng.uniform(10.0, 100.0, (ncol, nlyr))
    ext0 = rng.uniform(0.0, 1.0, (nwave, ncol, nlyr))
    worst = 0.0
    for kind in ("wavelength", "wavenumber"):
        coord = x if kind == "wavelength" else 1.0e4 / x
        kw = {kind: torch.as_tensor(coord, device=DEV)}
        rkw = {kind: coord}
        tag = f"{nwave}x{ncol}x{nlyr} nsp={nsp} {kind}"
        # one attenuator
        for i in (0, 1):
            wl, kd, sp, _ = T.ref[i]
            _, got, ref = _both(lambda conc: T.atts[i].forward(conc, kw),
                                lambda conc: ogr.attenuate(wl, kd, sp, conc, **rkw),
                                dict(conc=_conc(rng, ncol, nlyr, nsp, True)), rng)
            worst = max(worst, _compare(f"{tag} attenuate[{i}]", got, ref))
        # band_optics
        t3 = [t[:3] for t in T.ref]
        conc = _conc(rng, ncol, nlyr, nsp, False)
        out, got, ref = _both(lambda conc, dz: band_optics(T.atts, conc, dz, kw, nprop=3),
                              lambda conc, dz: ogr.band_optics(t3, conc, dz, 3, **rkw),
                              dict(conc=conc, dz=dz), rng)
        assert (out[:, ncol - 1, 0, :2] == 0.0).all()  # the layer without extinction
        worst = max(worst, _compare(f"{tag} band_optics", got, ref))
        # band_loop_optics
        for nmom, e0 in ((0, None), (8, ext0), (32, None), (8, None)):
            inputs = dict(conc=_conc(rng, ncol, nlyr, nsp, True), dz=dz)
            if e0 is not None:
                inputs["ext0"] = e0
            _, got, ref = _both(
                lambda **a: band_loop_optics(T.atts, a["conc"], a["dz"], kw, nmom, a.get("ext0")),
                lambda **a: ogr.band_loop_optics(T.ref, a["conc"], a["dz"], nmom,
                                                 ext0=a.get("ext0"), **rkw), inputs, rng)
            worst = max(worst, _compare(f"{tag} band_loop nmom={nmom} ext0={e0 is not None}",
                                        got, ref))
    print(f"optics grad tables {nwave}x{ncol}x{nlyr} nsp={nsp}: worst {worst:.3e}")
    assert margin(worst) < TOL
    assert worst < TIGHT, worst


# ---- RFM -----------------------------------------------------------------------------------
def _rfm_table(rng, nwave, inner):
    """descending pressures with 1 Pa (ln p = 0 exactly, in numpy, torch and on the device
    alike) as the last knot or, with `inner`, as an inner one"""
    pres = np.array([1.0e5, 1.0e3, 1.0, 1.0e-3]) if inner else np.array([1.0e5, 1.0e3, 10.0, 1.0])
    return dict(wave=np.linspace(10.0, 1500.0, nwave) if nwave > 1 else np.array([50.0]),
                pres=pres, lnp=np.log(pres), tgrid=np.linspace(-40.0, 40.0, 5),
                tref=np.array([320.0, 260.0, 200.0, 150.0]),
                kdata=rng.uniform(-4.0, 2.0, (nwave, 4, 5)))


def _rfm_module(tab, species):
    from pyharp_amd.opacity import RFM
    return RFM.from_arrays(tab["wave"], tab["pres"], tab["tgrid"], tab["tref"], tab["kdata"],
                           species=species)


def _tref(tab, p):
    return harp_np.interpn([np.log(p)], tab["tref"], [tab["lnp"]])


def _rfm_state(rng, tab, ncol, nlyr, nsp, species):
    """random (p, T) inside the grid; then, as far as ncol * nlyr goes: p on the 1 Pa knot
    with T on an inner, the last and the first anomaly knot; p above the table; p below it
    with T above the anomaly grid; T below the anomaly grid; conc exactly 0"""
    n = ncol * nlyr
    pres = np.exp(rng.uniform(np.log(2.0), np.log(5.0e4), n))
    anom = rng.uniform(-38.0, 38.0, n)
    special = ((1.0, 0.0), (1.0, 40.0), (1.0e7, 7.0), (1.0e-4, 60.0), (None, -60.0), (1.0, -40.0))
    for i, (p, a) in enumerate(special[:n]):
        if p is not None:
            pres[i] = p
        anom[i] = a
    temp = np.array([_tref(tab, p) for p in pres]) + anom
    for i, (p, a) in enumerate(special[:n]):  # the knots are hit exactly, not nearly
        if p == 1.0 and tab["lnp"][-1] == 0.0:
            assert temp[i] - _tref(tab, pres[i]) == a and a in tab["tgrid"]
        if p == 1.0:
            assert np.log(pres[i]) == 0.0 and 0.0 in tab["lnp"]
    conc = rng.uniform(0.05, 2.0, (ncol, nlyr, nsp))
    conc.reshape(n, nsp)[n - 1, species] = 0.0
    return conc, pres.reshape(ncol, nlyr), temp.reshape(ncol, nlyr)


@pytest.mark.parametrize("nsp", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rfm_parity_with_the_judge(shape, nsp):
    nwave, ncol, nlyr = shape
    rng = np.random.default_rng(2000 * nwave + 10 * ncol + nsp)
    species = nsp - 1
    tab = _rfm_table(rng, nwave, inner=nsp == 3)
    rfm = _rfm_module(tab, species)
    conc, pres, temp = _rfm_state(rng, tab, ncol, nlyr, nsp, species)
    _, got, ref = _both(
        lambda conc, pres, temp: rfm.forward(conc, {"pres": pres, "temp": temp}),
        lambda conc, pres, temp: ogr.rfm_forward(tab["wave"], tab["lnp"], tab["tgrid"],
                                                 tab["tref"], tab["kdata"], conc, pres, temp,
                                                 species),
        dict(conc=conc, pres=pres, temp=temp), rng)
    worst = _compare(f"{nwave}x{ncol}x{nlyr} nsp={nsp} rfm", got, ref)
    n = ncol * nlyr
    assert got["conc"].reshape(n, nsp)[n - 1, species] != 0.0  # d/dc at c = 0
    if nsp == 3:
        assert (got["conc"][..., :2] == 0.0).all()  # species the table does not read
    print(f"optics grad rfm {nwave}x{ncol}x{nlyr} nsp={nsp}: worst {worst:.3e}")
    assert margin(worst) < TOL
    assert worst < TIGHT, worst


# ---- 2: the reduction order ------------------------------------------------------------------
NCOL_MANY, COL = 3000, 1234  # 3 and 9 000 (col, lyr): either side of the launcher's one switch


def _grads(fn, inputs, cot):
    leaves = {k: v.clone().requires_grad_() for k, v in inputs.items()}
    fn(**leaves).backward(cot)
    return {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize("nwave", [2 * WB + 3, 1000])
def test_a_column_alone_and_among_3000_gives_the_same_bits(nwave, tables):
    from pyharp_amd.opacity import band_loop_optics, band_optics
    nlyr, nsp = 3, 3
    T = tables[nsp]
    gen = torch.Generator(device=DEV).manual_seed(5 + nwave)

    def rand(*shape, lo=0.0, hi=1.0):
        return lo + (hi - lo) * torch.rand(shape, dtype=torch.float64, device=DEV, generator=gen)

    rng = np.random.default_rng(77)
    kw = {"wavelength": torch.as_tensor(_coords(rng, T, nwave), device=DEV)}
    conc, dz = rand(NCOL_MANY, nlyr, nsp, lo=0.05, hi=2.0), rand(NCOL_MANY, nlyr, lo=10.0, hi=100.0)
    ext0 = rand(nwave, NCOL_MANY, nlyr)
    tab = _rfm_table(rng, nwave, inner=True)
    rfm = _rfm_module(tab, 1)
    pres = torch.exp(rand(NCOL_MANY, nlyr, lo=np.log(2.0), hi=np.log(5.0e4)))
    temp = rand(NCOL_MANY, nlyr, lo=160.0, hi=300.0)
    one = slice(COL, COL + 1)
    calls = (
        ("attenuate", lambda conc: T.atts[1].forward(conc, kw), dict(conc=conc), {}, 2),
        ("band_optics", lambda conc, dz: band_optics(T.atts, conc, dz, kw), dict(conc=conc, dz=dz),
         {}, 2),
        ("band_loop", lambda conc, dz, ext0: band_loop_optics(T.atts, conc, dz, kw, 2, ext0),
         dict(conc=conc, dz=dz), dict(ext0=ext0), 4),
        ("rfm", lambda conc, pres, temp: rfm.forward(conc, {"pres": pres, "temp": temp}),
         dict(conc=conc, pres=pres, temp=temp), {}, 1))
    for name, fn, per_col, per_wave, nslot in calls:
        cot = rand(nwave, NCOL_MANY, nlyr, nslot, lo=-1.0, hi=1.0)
        many = _grads(fn, {**per_col, **per_wave}, cot)
        again = _grads(fn, {**per_col, **per_wave}, cot)
        alone = _grads(fn, {**{k: v[one].contiguous() for k, v in per_col.items()},
                            **{k: v[:, one].contiguous() for k, v in per_wave.items()}},
                       cot[:, one].contiguous())
        for k in per_col:
            assert torch.equal(many[k], again[k]), (name, k)
            assert torch.equal(many[k][one], alone[k]), (name, k)
        for k in per_wave:
            assert torch.equal(many[k][:, one], alone[k]), (name, k)


def test_one_wave_of_ones_is_the_closed_form(tmp_path):
    """k = 2, ssa = 1/2 at every wavelength, one wave, gout = 1: d/dc = k (1 + ssa) = 3"""
    T = _Tables(tmp_path, 3, const=True)
    conc = _leaf(np.random.default_rng(3).uniform(0.1, 1.0, (5, 4, 3)))
    out = T.atts[0].forward(conc, {"wavelength": torch.tensor([1.3], dtype=torch.float64,
                                                               device=DEV)})
    out.backward(torch.ones_like(out))
    want = torch.zeros_like(conc)
    want[..., 1] = 3.0
    assert torch.equal(conc.grad, want)


# ---- 3: partial requests ---------------------------------------------------------------------
def _subsets(names):
    return [s for r in range(1, len(names)) for s in itertools.combinations(names, r)]


def _partial(fn, inputs):
    """every proper subset of the inputs requiring grad gives the bits of the full request;
    an input that does not require grad gets None"""
    leaves = {k: _leaf(v) for k, v in inputs.items()}
    out = fn(**leaves)
    cot = torch.as_tensor(np.random.default_rng(8).uniform(-1, 1, tuple(out.shape)), device=DEV)
    out.backward(cot)
    full = {k: v.grad for k, v in leaves.items()}
    for sub in _subsets(tuple(inputs)):
        part = {k: _leaf(v, grad=k in sub) for k, v in inputs.items()}
        fn(**part).backward(cot)
        for k, v in part.items():
            if k in sub:
                assert torch.equal(v.grad, full[k]), (sub, k)
            else:
                assert v.grad is None, (sub, k)


@pytest.mark.parametrize("ncol", [2, 400])  # the few-column and the many-column route
def test_partial_requests_give_the_same_bits(ncol, tables):
    from pyharp_amd.opacity import band_loop_optics, band_optics
    nwave, nlyr, nsp = 2 * WB + 3, 24, 3
    T = tables[nsp]
    rng = np.random.default_rng(91)
    kw = {"wavenumber": torch.as_tensor(1.0e4 / _coords(rng, T, nwave), device=DEV)}
    conc, dz = _conc(rng, ncol, nlyr, nsp, True), rng.uniform(10.0, 100.0, (ncol, nlyr))
    _partial(lambda conc, dz: band_optics(T.atts, conc, dz, kw), dict(conc=conc, dz=dz))
    _partial(lambda conc, dz, ext0: band_loop_optics(T.atts, conc, dz, kw, 8, ext0),
             dict(conc=conc, dz=dz, ext0=rng.uniform(0.0, 1.0, (nwave, ncol, nlyr))))
    tab = _rfm_table(rng, nwave, inner=True)
    rfm = _rfm_module(tab, 2)
    conc, pres, temp = _rfm_state(rng, tab, ncol, nlyr, nsp, 2)
    _partial(lambda conc, pres, temp: rfm.forward(conc, {"pres": pres, "temp": temp}),
             dict(conc=conc, pres=pres, temp=temp))


def test_broadcast_inputs_get_their_gradient_summed(tables):
    """dz (nlyr,) and pres / temp (nlyr,) enter through expand: torch sums over the columns"""
    from pyharp_amd.opacity import band_optics
    T = tables[3]
    rng = np.random.default_rng(92)
    nwave, ncol, nlyr = 5, 3, 4
    kw = {"wavelength": torch.as_tensor(_coords(rng, T, nwave), device=DEV)}
    conc = torch.as_tensor(rng.uniform(0.1, 1.0, (ncol, nlyr, 3)), device=DEV)
    dz1 = _leaf(rng.uniform(10.0, 100.0, nlyr))
    dz2 = _leaf(dz1.detach().expand(ncol, nlyr).cpu().numpy())
    cot = torch.as_tensor(rng.uniform(-1, 1, (nwave, ncol, nlyr, 2)), device=DEV)
    band_optics(T.atts, conc, dz1, kw).backward(cot)
    band_optics(T.atts, conc, dz2, kw).backward(cot)
    assert dz1.grad.shape == (nlyr,)
    assert torch.allclose(dz1.grad, dz2.grad.sum(0), rtol=1e-14, atol=0.0)
    tab = _rfm_table(rng, nwave, inner=True)
    rfm = _rfm_module(tab, 0)
    p1, t1 = _leaf(rng.uniform(10.0, 1.0e4, nlyr)), _leaf(rng.uniform(180.0, 300.0, nlyr))
    out = rfm.forward(conc, {"pres": p1, "temp": t1})
    out.backward(torch.ones_like(out))
    assert p1.grad.shape == (nlyr,) and t1.grad.shape == (nlyr,) and bool((t1.grad != 0).any())


# ---- 4: argument checks ----------------------------------------------------------------------
def test_the_adjoints_refuse_what_their_forwards_refuse(tables):
    from pyharp_amd import _lib
    lib = _lib.load()
    T = tables[3]
    nwave, ncol, nlyr, nsp = 4, 2, 3, 3
    ones = torch.ones(4096, dtype=torch.float64, device=DEV)  # every input
    zero = torch.zeros(4096, dtype=torch.float64, device=DEV)  # every cotangent
    buf = torch.zeros(4096, dtype=torch.float64, device=DEV)   # every output
    i, z, o = ones.data_ptr(), zero.data_ptr(), buf.data_ptr()
    att = T.atts[0].hd_struct(DEV)
    atts = (_lib.HdAttenuator * 2)(T.atts[0].hd_struct(DEV), T.atts[2].hd_struct(DEV))
    batts = (_lib.HdBandAttenuator * 1)(_lib.HdBandAttenuator(table=att, gasym=None))
    tab = _rfm_module(_rfm_table(np.random.default_rng(1), nwave, True), 1).hd_struct(DEV)
    torch.cuda.synchronize()
    ok = dict(att=(ctypes.byref(att), i, 0, nwave, i, ncol, nlyr, nsp, z, o, None),
              band=(atts, 2, i, 0, nwave, i, ncol, nlyr, nsp, i, 2, z, o, o, None),
              loop=(batts, 1, None, i, 0, nwave, i, ncol, nlyr, nsp, i, 0, z, o, o, None, None),
              rfm=(ctypes.byref(tab), i, ncol, nlyr, nsp, i, i, z, o, o, o, None))
    fn = dict(att=lib.hd_attenuate_bwd, band=lib.hd_band_optics_bwd,
              loop=lib.hd_band_loop_optics_bwd, rfm=lib.hd_rfm_attenuate_bwd)

    def call(which, **change):
        a = list(ok[which])
        for k, v in change.items():
            a[int(k[1:])] = v
        return fn[which](*a)

    for which in ok:  # the unchanged calls are accepted (a zero cotangent: zeros out)
        assert call(which) == 0, (which, _lib.last_error())
    # species out of range (nspecies below the species the tables read)
    assert call("att", _7=1) == EINVAL and call("band", _8=1) == EINVAL
    assert call("loop", _9=1) == EINVAL and call("rfm", _4=1) == EINVAL
    # natt 0, a bad coordinate kind
    assert call("band", _1=0) == EINVAL and call("loop", _1=0) == EINVAL
    assert call("att", _2=7) == EINVAL and call("band", _3=7) == EINVAL
    assert call("loop", _4=7) == EINVAL
    # a null cotangent with work to do
    assert call("att", _8=None) == EINVAL and call("band", _11=None) == EINVAL
    assert call("loop", _12=None) == EINVAL and call("rfm", _7=None) == EINVAL
    torch.cuda.synchronize()
    assert (buf == 0.0).all()  # the refused calls wrote nothing


# ---- 5: the epilogue ---------------------------------------------------------------------------
def test_band_sums_against_the_judge():
    from pyharp_amd.spectral import band_flux, band_flx, band_rad
    rng = np.random.default_rng(61)
    w = rng.uniform(0.1, 2.0, 17)
    wd = torch.as_tensor(w, device=DEV)
    worst = 0.0
    for fn, shape in ((band_flux, (17, 3, 5, 2)), (band_flx, (17, 3, 5, 8)), (band_rad, (17, 3, 5, 4))):
        x = rng.uniform(-1.0, 1.0, shape)
        out, got, ref = _both(lambda x: fn(x, wd), lambda x: ogr.band_sum(x, w), dict(x=x), rng)
        worst = max(worst, _compare(fn.__name__, got, ref))
        with pytest.raises(RuntimeError, match="weights requires grad"):
            fn(_leaf(x), _leaf(w))
        with pytest.raises(RuntimeError, match="out=.*requires grad"):
            fn(_leaf(x), wd, out=torch.empty(shape[1:], dtype=torch.float64, device=DEV))
    assert margin(worst) < TOL
    assert worst < TIGHT, worst


@pytest.mark.parametrize("nlyr", [1, 5])
def test_heating_rate_against_the_judge(nlyr):
    from pyharp_amd.spectral import heating_rate
    rng = np.random.default_rng(62 + nlyr)
    inputs = dict(bflux=rng.uniform(1.0, 90.0, (3, nlyr + 1, 2)),
                  dz=rng.uniform(100.0, 2000.0, (3, nlyr)), rho=rng.uniform(0.01, 1.5, (3, nlyr)))
    _, got, ref = _both(lambda bflux, dz, rho: heating_rate(bflux, dz, rho, 844.0),
                        lambda bflux, dz, rho: ogr.heating_rate(bflux, dz, rho, 844.0), inputs, rng)
    worst = _compare(f"heating_rate nlyr={nlyr}", got, ref)
    assert margin(worst) < TOL
    assert worst < TIGHT, worst
    # dz and rho per layer: summed over the columns by torch
    dz1, rho1 = _leaf(inputs["dz"][0]), _leaf(inputs["rho"][0])
    heating_rate(_leaf(inputs["bflux"], grad=False), dz1, rho1, 844.0).sum().backward()
    assert dz1.grad.shape == (nlyr,) and rho1.grad.shape == (nlyr,)


# ---- 6: the chain state -> optics -> solver ----------------------------------------------------
def _chain_case():
    rng = np.random.default_rng(2024)
    nwave, ncol, nlyr = 24, 3, 7
    tab = dict(wave=np.linspace(100.0, 1400.0, nwave), pres=np.logspace(5, 0, 8),
               tgrid=np.linspace(-40.0, 40.0, 5), tref=np.linspace(300.0, 160.0, 8))
    tab["lnp"] = np.log(tab["pres"])
    kd = [rng.uniform(-2.0, 5.0, (nwave, 8, 5)) for _ in range(2)]  # layers thin to tau ~ 4
    pres = np.exp(rng.uniform(np.log(5.0), np.log(5.0e4), (ncol, nlyr)))
    temp = np.array([[_tref(tab, p) for p in row] for row in pres]) + rng.uniform(-30, 30, (ncol, nlyr))
    state = dict(conc=rng.uniform(0.5, 30.0, (ncol, nlyr, 2)), pres=pres, temp=temp)
    bc = {"albedo": rng.uniform(0, 1, (nwave, ncol)), "fisot": rng.uniform(0, 0.1, (nwave, ncol)),
          "btemp": rng.uniform(250, 300, (nwave, ncol)), "ttemp": rng.uniform(100, 200, (nwave, ncol)),
          "temis": rng.uniform(0.1, 0.9, (nwave, ncol))}
    lo = np.sort(rng.uniform(100, 1500, nwave))
    hi = lo + rng.uniform(10, 300, nwave)
    extra = dict(w=rng.uniform(0.1, 2.0, nwave),
                 umu=np.array([-1.0, -0.3, 0.05, 0.37, 1.0]),
                 dz=rng.uniform(100.0, 2000.0, (ncol, nlyr)), rho=rng.uniform(0.01, 1.5, (ncol, nlyr)))
    return tab, kd, state, bc, lo, hi, extra


@pytest.mark.parametrize("loss", ["rays_band", "heating"])
def test_chain_from_the_state_to_the_observation(loss):
    from pyharp_amd import BeerLambert, BeerLambertOptions, layer2level
    from pyharp_amd.spectral import heating_rate
    tab, kd, state, bc, lo, hi, ex = _chain_case()
    nwave, (ncol, nlyr) = len(lo), state["pres"].shape
    op = BeerLambertOptions().nstr(8).nlyr(nlyr).nwave(nwave).ncol(ncol).planck(True) \
        .wave_lower(list(map(float, lo))).wave_upper(list(map(float, hi)))
    solver = BeerLambert(op)
    mods = [_rfm_module(dict(tab, kdata=k), i) for i, k in enumerate(kd)]
    cot = np.random.default_rng(5).uniform(-1, 1, (ncol, 5) if loss == "rays_band" else (ncol, nlyr))

    def run(dev, gpu):
        s = {k: _leaf(v, dev) for k, v in state.items()}
        t = lambda x: torch.as_tensor(x, dtype=torch.float64, device=dev)  # noqa: E731
        bcs = {k: t(v) for k, v in bc.items()}
        if gpu:
            kw = {"pres": s["pres"], "temp": s["temp"]}
            prop = mods[0](s["conc"], kw) + mods[1](s["conc"], kw)
        else:
            prop = sum(ogr.rfm_forward(tab["wave"], tab["lnp"], tab["tgrid"], tab["tref"], k,
                                       s["conc"], s["pres"], s["temp"], i) for i, k in enumerate(kd))
        temf = layer2level(s["temp"])
        rkw = dict(nstr=8, planck=True, wave_lower=lo, wave_upper=hi)
        if loss == "rays_band":
            if gpu:
                out = solver.forward_rays_band(prop, bcs, temf, umu=t(ex["umu"]), weights=t(ex["w"]))
            else:
                out = ogr.band_sum(beer_grad_ref.beer_rays(prop, bcs, temf, umu=ex["umu"], **rkw),
                                   ex["w"])
        else:
            if gpu:
                bflux = solver.forward_band(prop, bcs, temf, weights=t(ex["w"]))
                out = heating_rate(bflux, t(ex["dz"]), t(ex["rho"]), 844.0)
            else:
                out = ogr.heating_rate(ogr.band_sum(beer_grad_ref.beer_flux(prop, bcs, temf, **rkw),
                                                    ex["w"]), ex["dz"], ex["rho"], 844.0)
        out.backward(t(cot))
        return out.detach(), {k: v.grad for k, v in s.items()}

    out, got = run(DEV, True)
    rout, ref = run(CPU, False)
    fwd = np.abs(out.cpu().numpy() - rout.numpy()).max() / np.abs(rout.numpy()).max()
    assert fwd < 1e-9, fwd
    worst = _compare(f"chain {loss}", got, ref)
    assert margin(worst) < TOL


# ---- 7: CPU tensors ------------------------------------------------------------------------------
def test_cpu_tensors_get_cpu_gradients_equal_to_the_device_run(tables):
    from pyharp_amd.opacity import band_loop_optics
    T = tables[3]
    rng = np.random.default_rng(93)
    nwave, ncol, nlyr, nsp = 2 * WB + 3, 2, 5, 3
    x = _coords(rng, T, nwave)
    tab = _rfm_table(rng, nwave, inner=True)
    rfm = _rfm_module(tab, 1)
    conc, pres, temp = _rfm_state(rng, tab, ncol, nlyr, nsp, 1)
    dz, ext0 = rng.uniform(10.0, 100.0, (ncol, nlyr)), rng.uniform(0.0, 1.0, (nwave, ncol, nlyr))
    for fn, inputs in (
            (lambda dev, conc, pres, temp: rfm.forward(conc, {"pres": pres, "temp": temp}),
             dict(conc=conc, pres=pres, temp=temp)),
            (lambda dev, conc, dz, ext0: band_loop_optics(
                T.atts, conc, dz, {"wavelength": torch.as_tensor(x, device=dev)}, 8, ext0),
             dict(conc=conc, dz=dz, ext0=ext0)),
            (lambda dev, conc: T.atts[1].forward(conc, {"wavelength": torch.as_tensor(x, device=dev)}),
             dict(conc=conc))):
        grads = {}
        for dev in (CPU, DEV):
            leaves = {k: _leaf(v, dev) for k, v in inputs.items()}
            out = fn(dev, **leaves)
            cot = torch.as_tensor(np.random.default_rng(9).uniform(-1, 1, tuple(out.shape)),
                                  device=out.device)
            out.backward(cot)
            grads[dev] = {k: v.grad for k, v in leaves.items()}
        for k in inputs:
            assert grads[CPU][k].device.type == "cpu" and grads[DEV][k].device.type == "cuda"
            assert torch.equal(grads[CPU][k], grads[DEV][k].cpu()), k
