"""Raw output bytes of the library on seeded inputs, for a byte-for-byte comparison of two
builds (this tree's and another commit's) on one GPU.

    HD_LIB_PATH=/path/to/other/libhdisort.so python scripts/bitwise_outputs.py dump OUT_A
    python scripts/bitwise_outputs.py dump OUT_B          # the in-tree library
    python scripts/bitwise_outputs.py compare OUT_A OUT_B # "equal|DIFFERENT bytes name", a count

Each dump is one fresh process (a process loads one library); every output goes to
OUT/<case>.bin.  compare exits 1 when a case differs or exists on one side only.
profiles/retire/bitwise_vs_parent.txt is compare's output; the case list there says what
the names mean.
"""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WL = [100.0, 400.0, 700.0, 1000.0, 1300.0, 1600.0]
WU = [300.0, 600.0, 900.0, 1200.0, 1500.0, 1800.0]


def _inputs(rng, nwave, ncol, nlyr, nstr, planck, beam):
    prop = np.zeros((nwave, ncol, nlyr, 2 + nstr))
    prop[..., 0] = 10.0 ** rng.uniform(-3.0, 0.7, (nwave, ncol, nlyr))
    prop[..., 1] = rng.uniform(0.0, 0.99, (nwave, ncol, nlyr))
    gg = rng.uniform(0.0, 0.8, (nwave, ncol, nlyr))
    for l in range(nstr):
        prop[..., 2 + l] = gg ** (l + 1)
    bc = {"albedo": rng.uniform(0, 1, (nwave, ncol)), "fisot": np.full((nwave, ncol), 0.01)}
    if beam:
        bc.update(fbeam=rng.uniform(0.5, 2, (nwave, ncol)), umu0=rng.uniform(0.1, 1, (nwave, ncol)),
                  phi0=rng.uniform(0, 360, (nwave, ncol)))
    temf = None
    if planck:
        temf = np.linspace(180.0, 290.0, nlyr + 1)[::-1][None, :] + rng.uniform(-5, 5, (ncol, nlyr + 1))
        bc.update(btemp=np.full((nwave, ncol), 295.0), ttemp=np.full((nwave, ncol), 150.0),
                  temis=np.full((nwave, ncol), 0.3))
    return prop, bc, temf


def dump(out_dir):
    import torch
    from pyharp_amd import BeerLambert, BeerLambertOptions, Disort, DisortOptions
    from pyharp_amd.disort import _context
    import hard_cases

    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device("cuda", 0)
    ctx = _context(0)

    def t(x, where=dev):
        return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64,
                                                      device=where)

    def tb(bc, where=dev):
        return {k: t(v, where) for k, v in bc.items()}

    def save(name, x):
        torch.cuda.synchronize()
        x.detach().cpu().numpy().tofile(os.path.join(out_dir, name + ".bin"))

    def disort(nstr, nlyr, nwave, ncol, planck, flags="lamber,quiet,onlyfl", nmom=None, radius=None,
               wl=None, wu=None, **opts):
        op = DisortOptions().flags(flags + (",planck" if planck else "")).nwave(nwave).ncol(ncol)
        if planck:
            op.wave_lower(list(wl or WL[:nwave])).wave_upper(list(wu or WU[:nwave]))
        if radius is not None:
            op.radius(radius)
        for k, v in opts.items():
            getattr(op, k)(list(v))
        op.ds().nlyr = nlyr
        op.ds().nstr = nstr
        op.ds().nmom = nstr if nmom is None else nmom
        return Disort(op)

    # ---- the flux entry points: forward, forward_band (with and without kept fluxes), flx
    nwave, ncol, nlyr = 5, 13, 9
    for nstr in (4, 8, 16, 20, 32):
        for planck in (0, 1):
            for beam in (0, 1):
                rng = np.random.default_rng(1000 * nstr + 10 * planck + beam)
                prop, bc, temf = _inputs(rng, nwave, ncol, nlyr, nstr, planck, beam)
                w = t(rng.uniform(0.1, 2.0, nwave))
                d = disort(nstr, nlyr, nwave, ncol, planck)
                a = (t(prop), tb(bc), t(temf))
                for chunk in (0, 7, 33):
                    tag = f"n{nstr}_p{planck}_b{beam}_c{chunk}"
                    ctx.set_chunk(chunk)
                    try:
                        save("forward_" + tag, d.forward(*a))
                        save("band_" + tag, d.forward_band(*a, weights=w))
                        keep = torch.full((nwave, ncol, nlyr + 1, 2), -1.0, dtype=torch.float64,
                                          device=dev)
                        save("bandkeep_" + tag, d.forward_band(*a, weights=w, flux=keep))
                        save("bandkeepflux_" + tag, keep)
                        save("flx_" + tag, d.forward_flx(*a))
                    finally:
                        ctx.set_chunk(0)

    # ---- a chunk of at least 4 096 solves on the team path: the nontemporal instantiations
    # of its layer kernel and sweep (4 099 solves of two layers, a last team of three)
    for nstr in (18, 32):
        rng = np.random.default_rng(4099 + nstr)
        prop, bc, temf = _inputs(rng, 1, 4099, 2, nstr, 1, 1)
        d = disort(nstr, 2, 1, 4099, 1)
        st = torch.zeros(4099, dtype=torch.int32, device=dev)
        save(f"forward_nt_n{nstr}", d.forward(t(prop), tb(bc), t(temf), status=st))
        save(f"forward_nt_n{nstr}_status", st)
    # the same on the one-lane path (nstr 6 and 16: at 4 and 8 a chunk this small runs the quad
    # sweep): the nontemporal layer kernel, sweep and back-substitution, plain, with the
    # pseudo-spherical beam, and with it and the second functional
    for nstr in (6, 16):
        rng = np.random.default_rng(4099 + nstr)
        prop, bc, temf = _inputs(rng, 1, 4099, 2, nstr, 1, 1)
        a = (t(prop), tb(bc), t(temf))
        zd = t(np.linspace(0.0, 20.0e3, 3))
        d = disort(nstr, 2, 1, 4099, 1)
        ds = disort(nstr, 2, 1, 4099, 1, flags="lamber,quiet,onlyfl,spher", radius=3.39e6)
        for name, call in (("forward_nt", lambda st: d.forward(*a, status=st)),
                           ("spher_nt", lambda st: ds.forward(*a, zd=zd, status=st)),
                           ("flx_spher_nt", lambda st: ds.forward_flx(*a, zd=zd, status=st))):
            st = torch.zeros(4099, dtype=torch.int32, device=dev)
            save(f"{name}_n{nstr}", call(st))
            save(f"{name}_n{nstr}_status", st)
    del prop, bc, temf, a

    # ---- the smallest call on hd_solve_band's row-major route
    rng = np.random.default_rng(77)
    prop, bc, temf = _inputs(rng, 1, 131073, 4, 4, 0, 1)
    d = disort(4, 4, 1, 131073, 0)
    save("band_rowmajor", d.forward_band(t(prop), tb(bc), weights=t([1.5])))
    del prop, bc

    # ---- pseudo-spherical beam: one spher call and one forward_flx + spher call
    for nstr in (8, 24):
        rng = np.random.default_rng(4200 + nstr)
        prop, bc, temf = _inputs(rng, 3, 7, 9, nstr, 1, 1)
        zd = t(np.linspace(0.0, 90.0e3, 10))
        d = disort(nstr, 9, 3, 7, 1, flags="lamber,quiet,onlyfl,spher", radius=3.39e6)
        a = (t(prop), tb(bc), t(temf))
        save(f"spher_n{nstr}", d.forward(*a, zd=zd))
        save(f"flx_spher_n{nstr}", d.forward_flx(*a, zd=zd))
    # a low sun (secants that differ by layer, some negative under the thicker layers) on
    # altitudes per column, with the status words: no layer here is on a resonance
    for nstr in (4, 16, 32):
        rng = np.random.default_rng(4300 + nstr)
        prop, bc, temf = _inputs(rng, 2, 9, 12, nstr, 1, 1)
        bc["umu0"] = rng.uniform(0.01, 0.2, (2, 9))
        zd = t(np.linspace(0.0, 96.0e3, 13)[None, :] * rng.uniform(0.8, 1.2, (9, 1)))
        d = disort(nstr, 12, 2, 9, 1, flags="lamber,quiet,onlyfl,spher", radius=3.39e6)
        st = torch.zeros(18, dtype=torch.int32, device=dev)
        save(f"spher_lowsun_n{nstr}", d.forward(t(prop), tb(bc), t(temf), zd=zd, status=st))
        save(f"spher_lowsun_n{nstr}_status", st)

    # ---- the hard-regime fixture through forward
    fix = hard_cases.load(os.path.join(ROOT, "tests", "golden"))
    for (family, nstr), bs in sorted(fix.items()):
        if nstr not in (2, 16, 32):
            continue
        for b in bs:
            n = b["prop"].shape[1]
            d = disort(nstr, b["nlyr"], 1, n, b["planck"], nmom=b["nmom"],
                       wl=[hard_cases.WAVE[0]], wu=[hard_cases.WAVE[1]])
            st = torch.zeros(n, dtype=torch.int32, device=dev)
            save(f"hard_{family}_n{nstr}_{b['name']}",
                 d.forward(t(b["prop"]), tb(b["bc"]), t(b["temf"]), status=st))
            save(f"hard_{family}_n{nstr}_{b['name']}_status", st)

    # ---- radiances: the grid call, rays shared and per column, the ray band sum
    utau = [0.0, 0.05, 0.3, 1.0, 1.5]
    for nstr in (8, 24):
        rng = np.random.default_rng(300 + nstr)
        nwave, ncol, nlyr, nray = 2, 3, 6, 7
        prop, bc, temf = _inputs(rng, nwave, ncol, nlyr, nstr, 0, 1)
        prop[..., 0] = rng.uniform(0.3, 1.0, prop.shape[:3])  # every user depth inside
        umu = rng.uniform(0.1, 1.0, (ncol, nray)) * rng.choice([-1.0, 1.0], (ncol, nray))
        phi = rng.uniform(0.0, 360.0, (ncol, nray))
        a = (t(prop), tb(bc))
        flags = "lamber,quiet,usrtau,usrang"
        d = disort(nstr, nlyr, nwave, ncol, 0, flags=flags, user_tau=utau,
                   user_mu=sorted(umu[0]), user_phi=sorted(phi[0])[:3])
        save(f"radflux_n{nstr}", d.forward(*a))
        save(f"get_rad_n{nstr}", d.get_rad())
        d = disort(nstr, nlyr, nwave, ncol, 0, flags="lamber,quiet,usrtau", user_tau=utau)
        save(f"rays_shared_n{nstr}", d.forward_rays(*a, umu=t(umu[0]), phi=t(phi[0])))
        save(f"rays_percol_n{nstr}", d.forward_rays(*a, umu=t(umu), phi=t(phi)))
        save(f"rays_band_n{nstr}",
             d.forward_rays_band(*a, umu=t(umu), phi=t(phi), weights=t([0.7, 1.9])))

    # ---- radiances on the team path (nstr 18..32) with a Planck source: with a beam (every
    # azimuthal mode) and without (one mode); units = modes x nwave x ncol, the last a count
    # that is no multiple of the four units of a team block (54), as is the beamless one (6)
    for nstr, beam, nwave in ((18, 1, 2), (32, 1, 2), (18, 0, 2), (18, 1, 1)):
        rng = np.random.default_rng(7000 + 10 * nstr + 2 * beam + nwave)
        ncol, nlyr = 3, 6
        prop, bc, temf = _inputs(rng, nwave, ncol, nlyr, nstr, 1, beam)
        prop[..., 0] = rng.uniform(0.3, 1.0, prop.shape[:3])  # every user depth inside
        d = disort(nstr, nlyr, nwave, ncol, 1, flags="lamber,quiet,usrtau,usrang", user_tau=utau,
                   user_mu=[-1.0, -0.6, -0.15, 0.1, 0.45, 0.8], user_phi=[0.0, 75.0, 300.0])
        st = torch.zeros(nwave * ncol, dtype=torch.int32, device=dev)
        tag = f"n{nstr}_p1_b{beam}_w{nwave}"
        save("radflux_" + tag, d.forward(t(prop), tb(bc), t(temf), status=st))
        save("get_rad_" + tag, d.get_rad())
        save("radstatus_" + tag, st)

    # ---- the rest of the intensity path's routes: nstr 16 with Planck and a beam (the
    # user-angle maps' thermal vectors), fluxes at user depths only (nstr 8: the one-lane
    # kernels; 24: team layer and sweep, rolled const and flux), nstr 2 (NN = 1), per-column
    # rays at nstr 32 (the rolled user kernel)
    nwave, ncol, nlyr = 2, 3, 6
    umu6, phi3 = [-1.0, -0.6, -0.15, 0.1, 0.45, 0.8], [0.0, 75.0, 300.0]
    rng = np.random.default_rng(8016)
    prop, bc, temf = _inputs(rng, nwave, ncol, nlyr, 16, 1, 1)
    prop[..., 0] = rng.uniform(0.3, 1.0, prop.shape[:3])
    d = disort(16, nlyr, nwave, ncol, 1, flags="lamber,quiet,usrtau,usrang", user_tau=utau,
               user_mu=umu6, user_phi=phi3)
    save("radflux_n16_p1", d.forward(t(prop), tb(bc), t(temf)))
    save("get_rad_n16_p1", d.get_rad())
    for nstr in (8, 24):
        rng = np.random.default_rng(8100 + nstr)
        prop, bc, temf = _inputs(rng, nwave, ncol, nlyr, nstr, 1, 0)
        prop[..., 0] = rng.uniform(0.3, 1.0, prop.shape[:3])
        d = disort(nstr, nlyr, nwave, ncol, 1, flags="lamber,quiet,usrtau,onlyfl", user_tau=utau)
        save(f"onlyfl_utau_n{nstr}_p1", d.forward(t(prop), tb(bc), t(temf)))
    rng = np.random.default_rng(8002)
    prop, bc, temf = _inputs(rng, nwave, ncol, nlyr, 2, 0, 1)
    prop[..., 0] = rng.uniform(0.3, 1.0, prop.shape[:3])
    d = disort(2, nlyr, nwave, ncol, 0, flags="lamber,quiet,usrtau,usrang", user_tau=utau,
               user_mu=umu6, user_phi=phi3)
    d.forward(t(prop), tb(bc))
    save("get_rad_n2", d.get_rad())
    rng = np.random.default_rng(8032)
    prop, bc, temf = _inputs(rng, nwave, ncol, nlyr, 32, 0, 1)
    prop[..., 0] = rng.uniform(0.3, 1.0, prop.shape[:3])
    umu = rng.uniform(0.1, 1.0, (ncol, 7)) * rng.choice([-1.0, 1.0], (ncol, 7))
    phi = rng.uniform(0.0, 360.0, (ncol, 7))
    d = disort(32, nlyr, nwave, ncol, 0, flags="lamber,quiet,usrtau", user_tau=utau)
    save("rays_percol_n32", d.forward_rays(t(prop), tb(bc), umu=t(umu), phi=t(phi)))

    # ---- Beer-Lambert
    rng = np.random.default_rng(555)
    nstr, nlyr, nwave, ncol = 8, 17, 5, 11
    prop, bc, temf = _inputs(rng, nwave, ncol, nlyr, 0, 1, 0)

    def beer(alpha):  # alpha != 0 applies to the ray calls only
        op = BeerLambertOptions().alpha(alpha).nstr(nstr).nwave(nwave).ncol(ncol).nlyr(nlyr)
        op.planck(True).wave_lower(WL[:nwave]).wave_upper(WU[:nwave])
        return BeerLambert(op)

    b, br = beer(0.0), beer(0.5)
    a = (t(prop), tb(bc), t(temf))
    w = t(rng.uniform(0.1, 2.0, nwave))
    umu = t(rng.uniform(0.1, 1.0, 5) * np.array([1.0, -1.0, 1.0, -1.0, 1.0]))
    for chunk in (0, 7):
        ctx.set_chunk(chunk)
        try:
            save(f"beer_rays_band_c{chunk}", br.forward_rays_band(*a, umu=umu, weights=w))
            save(f"beer_rays_c{chunk}", br.forward_rays(*a, umu=umu))
            save(f"beer_flux_c{chunk}", b.forward(*a))
            save(f"beer_band_c{chunk}", b.forward_band(*a, weights=w))
        finally:
            ctx.set_chunk(0)

    # ---- host arrays in and out (hd_solve_band_host, hd_solve_host)
    cpu = torch.device("cpu")
    for nstr in (16, 32):
        rng = np.random.default_rng(900 + nstr)
        prop, bc, temf = _inputs(rng, 6, 9, 16, nstr, 0, 1)
        d = disort(nstr, 16, 6, 9, 0)
        save(f"band_host_n{nstr}", d.forward_band(t(prop, cpu), tb(bc, cpu),
                                                  weights=t(rng.uniform(0.1, 2.0, 6), cpu)))
    rng = np.random.default_rng(916)
    prop, bc, temf = _inputs(rng, 3, 17, 20, 16, 1, 1)
    d = disort(16, 20, 3, 17, 1)
    save("solve_host_n16_planck", d.forward(t(prop, cpu), tb(bc, cpu), t(temf, cpu)))
    print(f"{len(os.listdir(out_dir))} outputs in {out_dir}")


def compare(dir_a, dir_b):
    names = sorted(set(os.listdir(dir_a)) | set(os.listdir(dir_b)))
    bad = 0
    for n in names:
        pa, pb = os.path.join(dir_a, n), os.path.join(dir_b, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"ONE SIDE ONLY            {n[:-4]}")
            bad += 1
            continue
        a, b = open(pa, "rb").read(), open(pb, "rb").read()
        same = a == b and len(a) > 0
        bad += not same
        print(f"{'equal' if same else 'DIFFERENT':9s} {len(a):10d} bytes  {n[:-4]}")
    print(f"{len(names)} cases, {bad} different")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
