// hd_rad_spher.hip -- the nstr <= 16 one-lane intensity kernels with the pseudo-spherical
// beam (hd_solve_rays_spher, DESIGN.md sections 3b and 3e): hd_rad.hip compiled with
// HD_RAD_SPHER, which keeps its beam-using kernels (layer, sweep, const, flux, user_map and
// the ray epilogue with tms_sum / ims_term), puts them in hd::spher with tables of their
// own, and takes the beam of every layer from hd_spher_kernel's slant depths and secants
// (RadArgs::chp, lam, ch) instead of umu0.  The launch sequence stays hd_rad.hip's
// launch_rad_chunk, which takes these kernels through hd::spher::reg_kernels.
#define HD_RAD_SPHER 1
#include "hd_rad.hip"
