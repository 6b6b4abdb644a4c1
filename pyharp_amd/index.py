"""Layout constants of the optics / flux tensors (mirror of src/index.h:12-18)."""

# optical variables: prop[..., IEX] layer optical thickness, [..., ISS]
# single-scattering albedo, [..., IPM:] phase moments chi_1..chi_nmom
IEX = 0
ISS = 1
IPM = 2

# flux variables: flux[..., IUP] upward, [..., IDN] downward (rfldir + rfldn)
IUP = 0
IDN = 1

# full flux record of Disort.forward_flx / hd_solve_flx: flx[..., k], the component
# order of cdisort's disort_radiant (include/hdisort.h HD_FLX_*)
IRFLDIR = 0  # direct beam mu0 F0 exp(-tau/mu0), unscaled tau
IRFLDN = 1   # diffuse downward flux
IFLUP = 2    # upward flux
IDFDT = 3    # flux divergence (1 - ssa) 4 pi (uavg - B)
IUAVG = 4    # mean intensity
IUAVGDN = 5  # ... its downward diffuse part
IUAVGUP = 6  # ... its upward part
IUAVGSO = 7  # ... its direct-beam part (delta-M scaled depth)
NFLX = 8
