// opt_lds.hpp - the dynamic LDS of the K8a kernels of optimize.hip, written once: the kernels carve `smem` from these
// layouts and the host plan takes its byte counts from them (forward_plan, opt_forward_plan, ecckd_opt_create_ex), so the two
// sides cannot drift apart.  Plain constexpr C++ (no device-only code): tools/check_opt_tables.cpp includes it as it is.
// A layout is the byte offset of every array, in the order of its enum, and the total behind the last one; the double arrays
// come first, so every one of them starts on a multiple of 8.
#pragma once
#include <cstddef>

namespace ecckd {
namespace opt_lds {

template <int N>
struct Layout {
  size_t off[N + 1];
  constexpr size_t bytes() const { return off[N]; }
};

template <int N>
constexpr Layout<N> pack(const size_t (&size)[N]) {
  Layout<N> l{};
  for (int i = 0; i < N; ++i) l.off[i + 1] = l.off[i] + size[i];
  return l;
}

// k_opt_forward_adjoint_cells: T [nlay][ng] (longwave only) | D, U [nhl][ng] | bdn, bup [nhl][nband] | r [nlay][nband] |
// rsum [nlay] | sd, su [nhl] | red [16] | int bp [nband + 1] | int bg [ng]
enum CellsArray { CL_T, CL_D, CL_U, CL_BDN, CL_BUP, CL_R, CL_RSUM, CL_SD, CL_SU, CL_RED, CL_BP, CL_BG, CL_COUNT };
constexpr Layout<CL_COUNT> cells(int nlay, int ng, int nband, bool sw) {
  const size_t d = sizeof(double), nhl = (size_t)nlay + 1, flux = nhl * ng * d, band = nhl * nband * d;
  const size_t size[CL_COUNT] = {sw ? 0 : (size_t)nlay * ng * d, flux, flux, band, band, (size_t)nlay * nband * d, nlay * d, nhl * d, nhl * d,
                                 16 * d, ((size_t)nband + 1) * sizeof(int), (size_t)ng * sizeof(int)};
  return pack(size);
}

// k_opt_forward_adjoint_rayleigh: bdn, bup, gdn, gup [nhl][nband] | r [nlay][nband] | rsum [nlay] | sd, su [nhl] | red [16] |
// int bp [nband + 1] | int bg [ng]   (its <true> instance, the optimised Rayleigh coefficients, puts one double per thread
// behind this layout, from the next multiple of 8 bytes: ray_lds_offset and ray_lds_bytes of optimize.hip)
enum RayleighArray { RL_BDN, RL_BUP, RL_GDN, RL_GUP, RL_R, RL_RSUM, RL_SD, RL_SU, RL_RED, RL_BP, RL_BG, RL_COUNT };
constexpr Layout<RL_COUNT> rayleigh(int nlay, int ng, int nband) {
  const size_t d = sizeof(double), nhl = (size_t)nlay + 1, band = nhl * nband * d;
  const size_t size[RL_COUNT] = {band, band, band, band, (size_t)nlay * nband * d, nlay * d, nhl * d, nhl * d, 16 * d,
                                 ((size_t)nband + 1) * sizeof(int), (size_t)ng * sizeof(int)};
  return pack(size);
}

// k_opt_forward_adjoint_lw_angles: D, U [nhl][ng] the angle-summed fluxes | bdn, bup, gdn, gup [nhl][nband] | r [nlay][nband] |
// rsum [nlay] | sd, su [nhl] | red [16] | int bp [nband + 1] | int bg [ng]   (the per-angle state lives in a device workspace)
enum LwAnglesArray { AL_D, AL_U, AL_BDN, AL_BUP, AL_GDN, AL_GUP, AL_R, AL_RSUM, AL_SD, AL_SU, AL_RED, AL_BP, AL_BG, AL_COUNT };
constexpr Layout<AL_COUNT> lw_angles(int nlay, int ng, int nband) {
  const size_t d = sizeof(double), nhl = (size_t)nlay + 1, flux = nhl * ng * d, band = nhl * nband * d;
  const size_t size[AL_COUNT] = {flux, flux, band, band, band, band, (size_t)nlay * nband * d, nlay * d, nhl * d, nhl * d, 16 * d,
                                 ((size_t)nband + 1) * sizeof(int), (size_t)ng * sizeof(int)};
  return pack(size);
}

// k_opt_forward_adjoint (the general kernel): tau [nlay][ng] | fdn, fup [nhl][ng] | bdn, bup, gdn, gup [nhl][nband] | red [16] |
// unsigned char clamp [nlay][ng], rounded up to 16 bytes
enum GeneralArray { GL_TAU, GL_FDN, GL_FUP, GL_BDN, GL_BUP, GL_GDN, GL_GUP, GL_RED, GL_CLAMP, GL_COUNT };
constexpr Layout<GL_COUNT> general(int nlay, int ng, int nband) {
  const size_t d = sizeof(double), nhl = (size_t)nlay + 1, flux = nhl * ng * d, band = nhl * nband * d;
  const size_t size[GL_COUNT] = {(size_t)nlay * ng * d, flux, flux, band, band, band, band, 16 * d, ((size_t)nlay * ng + 15) / 16 * 16};
  return pack(size);
}

}  // namespace opt_lds
}  // namespace ecckd
