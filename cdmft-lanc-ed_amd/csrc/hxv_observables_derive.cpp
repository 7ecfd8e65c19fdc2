// The reference's named impurity observables from a raw record of hxv_observables_accumulate (include/hxv.h): host code only, no device.
// Every formula below is the reference's loop body with the per-basis-state occupations replaced by the impurity occupation histogram W
// (a basis state contributes its weight to exactly one W entry) and the hopping expectation values by R_up / R_dw.
#include <complex>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hxv.h"

namespace hxv {
int fail(int code, const std::string& msg);
}

namespace {
using cplx = std::complex<double>;

bool model_ok(const hxv_model* m) {
  return m && m->nlat >= 1 && m->norb >= 1 && m->norb <= 5 && (m->nspin == 1 || m->nspin == 2) && m->nlat * m->norb <= 10 && m->imphloc;
}
}  // namespace

extern "C" {

int64_t hxv_obs_derived_elems(const hxv_model* m) {
  if (!model_ok(m)) return 0;
  const int64_t L = m->nlat, O = m->norb, S = m->nspin;
  return 5 * L * O + 2 * L * L * O * O + L + 5 + 2 * L * L * S * S * O * O;
}

int hxv_observables_derive(const hxv_model* m, const double* record, double* out) {
  if (!model_ok(m) || !record || !out) return hxv::fail(HXV_ERR_ARG, "hxv_observables_derive: NULL argument or unsupported model (Nimp <= 10, Norb <= 5, Nspin 1 or 2)");
  const int L = m->nlat, O = m->norb, S = m->nspin, N = L * O;
  const int64_t nw = (int64_t)1 << N, nww = nw * nw, np = (int64_t)N * N;
  const double* W = record;
  const double* Rr[2] = {record + nww, record + nww + 2 * np};
  auto R = [&](int spin, int is, int js) { return cplx(Rr[spin][2 * (is + (int64_t)js * N)], Rr[spin][2 * (is + (int64_t)js * N) + 1]); };
  // impHloc(ilat,jlat,ispin,jspin,iorb,jorb), Fortran order, 0-based arguments
  auto H = [&](int il, int jl, int is, int js, int io, int jo) {
    const int64_t k = il + (int64_t)L * (jl + (int64_t)L * (is + (int64_t)S * (js + (int64_t)S * (io + (int64_t)O * jo))));
    return cplx(m->imphloc[2 * k], m->imphloc[2 * k + 1]);
  };
  const int64_t LO = (int64_t)L * O, LLOO = LO * LO;
  std::vector<double> dens(LO, 0.0), dup(LO, 0.0), ddw(LO, 0.0), docc(LO, 0.0), magz(LO, 0.0), sz2(LLOO, 0.0), n2(LLOO, 0.0), s2tot(L, 0.0);
  double eknot = 0.0, epot = 0.0, ehartree = 0.0, dust = 0.0, dund = 0.0;
  auto lo = [&](int il, int io) { return il + (int64_t)L * io; };                                                     // (Nlat,Norb)
  auto llo = [&](int il, int jl, int io, int jo) { return il + (int64_t)L * (jl + (int64_t)L * (io + (int64_t)O * jo)); };  // (Nlat,Nlat,Norb,Norb)
  std::vector<double> nu(N), nd(N), sz(N), nt(N);
  for (int64_t a = 0; a < nww; ++a) {
    const double w = W[a];
    if (w == 0.0) continue;
    for (int is = 0; is < N; ++is) {
      nu[is] = (double)((a >> is) & 1);
      nd[is] = (double)((a >> (N + is)) & 1);
      sz[is] = (nu[is] - nd[is]) / 2.0;
      nt[is] = nu[is] + nd[is];
    }
    // lanc_observables (ED_OBSERVABLES.f90:177-204); imp_state_index(ilat,iorb) = iorb + ilat*Norb (0-based)
    for (int il = 0; il < L; ++il) {
      double szs = 0.0;
      for (int io = 0; io < O; ++io) {
        const int is = io + il * O;
        dens[lo(il, io)] += nt[is] * w;
        dup[lo(il, io)] += nu[is] * w;
        ddw[lo(il, io)] += nd[is] * w;
        docc[lo(il, io)] += nu[is] * nd[is] * w;
        magz[lo(il, io)] += (nu[is] - nd[is]) * w;
        szs += sz[is];
      }
      s2tot[il] += szs * szs * w;
    }
    for (int il = 0; il < L; ++il)
      for (int io = 0; io < O; ++io) {
        const int is = io + il * O;
        sz2[llo(il, il, io, io)] += sz[is] * sz[is] * w;
        n2[llo(il, il, io, io)] += nt[is] * nt[is] * w;
        for (int jl = 0; jl < L; ++jl)
          for (int jo = io + 1; jo < O; ++jo) {
            sz2[llo(il, jl, io, jo)] += sz[io + il * O] * sz[jo + jl * O] * w;
            sz2[llo(il, jl, jo, io)] += sz[jo + il * O] * sz[io + jl * O] * w;
            n2[llo(il, jl, io, jo)] += nt[io + il * O] * nt[jo + jl * O] * w;
            n2[llo(il, jl, jo, io)] += nt[jo + il * O] * nt[io + jl * O] * w;
          }
      }
    // lanc_local_energy (:300-410): diagonal part of Eknot, Epot, Dust, Dund, Ehartree
    for (int il = 0; il < L; ++il)
      for (int io = 0; io < O; ++io) {
        const int is = io + il * O;
        eknot += (H(il, il, 0, 0, io, io) * nu[is] * w).real();
        eknot += (H(il, il, S - 1, S - 1, io, io) * nd[is] * w).real();
        epot += m->uloc[io] * nu[is] * nd[is] * w;
      }
    if (O > 1)
      for (int il = 0; il < L; ++il)
        for (int io = 0; io < O; ++io)
          for (int jo = io + 1; jo < O; ++jo) {
            const int is = io + il * O, js = jo + il * O;
            epot += m->ust * (nu[is] * nd[js] + nu[js] * nd[is]) * w;
            dust += (nu[is] * nd[js] + nu[js] * nd[is]) * w;
            epot += (m->ust - m->jh) * (nu[is] * nu[js] + nd[is] * nd[js]) * w;
            dund += (nu[is] * nu[js] + nd[is] * nd[js]) * w;
          }
    if (m->hfmode) {
      // DIVERGENCE from the reference: its constant term reads uloc(is), is = imp_state_index (:399), past Norb -- and for Nimp > 5 past the
      // 5-element Uloc (ED_INPUT_VARS.f90:19).  uloc(iorb) is the intent of the commented line at :395.
      for (int il = 0; il < L; ++il)
        for (int io = 0; io < O; ++io) {
          const int is = io + il * O;
          ehartree += -0.5 * m->uloc[io] * (nu[is] + nd[is]) * w + 0.25 * m->uloc[io] * w;
        }
      if (O > 1)
        for (int il = 0; il < L; ++il)
          for (int io = 0; io < O; ++io)
            for (int jo = io + 1; jo < O; ++jo) {
              const int is = io + il * O, js = jo + il * O;
              ehartree += -0.5 * m->ust * (nu[is] + nd[is] + nu[js] + nd[js]) * w + 0.25 * m->ust * w;
              ehartree += -0.5 * (m->ust - m->jh) * (nu[is] + nd[is] + nu[js] + nd[js]) * w + 0.25 * (m->ust - m->jh) * w;
            }
    }
  }
  // off-diagonal part of Eknot (:318-345): Re sum impHloc(ilat,jlat,s,s,iorb,jorb) * R_s(is,js), is != js; dw terms with impHloc(..,Nspin,Nspin,..)
  for (int il = 0; il < L; ++il)
    for (int jl = 0; jl < L; ++jl)
      for (int io = 0; io < O; ++io)
        for (int jo = 0; jo < O; ++jo) {
          const int is = io + il * O, js = jo + jl * O;
          if (is == js) continue;
          eknot += (H(il, jl, 0, 0, io, jo) * R(0, is, js)).real();
          eknot += (H(il, jl, S - 1, S - 1, io, jo) * R(1, is, js)).real();
        }
  epot += ehartree;  // :434
  double* o = out;
  for (const std::vector<double>* v : {&dens, &dup, &ddw, &docc, &magz, &sz2, &n2, &s2tot}) {
    std::memcpy(o, v->data(), v->size() * sizeof(double));
    o += v->size();
  }
  *o++ = eknot;
  *o++ = epot;
  *o++ = ehartree;
  *o++ = dust;
  *o++ = dund;
  // single_particle_density_matrix(ilat,jlat,ispin,ispin,iorb,jorb) = <c^+_is c_js> of spin ispin (:630-666); only ispin <= Nspin
  const int64_t nspdm = LLOO * S * S;
  std::memset(o, 0, 2 * nspdm * sizeof(double));
  for (int sp = 0; sp < S; ++sp)
    for (int il = 0; il < L; ++il)
      for (int jl = 0; jl < L; ++jl)
        for (int io = 0; io < O; ++io)
          for (int jo = 0; jo < O; ++jo) {
            const int64_t k = il + (int64_t)L * (jl + (int64_t)L * (sp + (int64_t)S * (sp + (int64_t)S * (io + (int64_t)O * jo))));
            const cplx r = R(sp, io + il * O, jo + jl * O);
            o[2 * k] = r.real();
            o[2 * k + 1] = r.imag();
          }
  return HXV_OK;
}

}  // extern "C"
