/*
 * hxv_oracle.c -- CPU restatement (plain C99) of the reference's stored-sparse
 * sector Hamiltonian x vector path.  TEST INFRASTRUCTURE ONLY.
 *
 *   Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 *   load this library, and only as the checker / timed CPU baseline.  The
 *   product (cdmft-lanc-ed_amd/) never links, imports or calls it.
 *
 * What is restated (reference = QcmPlab/CDMFT-LANC-ED @ 2024_08_07, paths
 * relative to /root/reference):
 *   - sector maps            ED_SETUP.f90:720-775 (build_sector)
 *   - c / cdg / bdecomp      ED_SETUP.f90:807-833, :935-945
 *   - binary_search          ED_SETUP.f90:1044-1061
 *   - bath stride / indices  ED_SETUP.f90:367-375, :547-568; ED_AUX_FUNX.f90:81-87
 *   - row-list sparse matrix ED_SPARSE_MATRIX.f90:13-30, :254-322 (append, dup = sum)
 *   - ed_buildh_main         ED_HAMILTONIAN_SPARSE_HxV.f90:40-152
 *       H_local              ED_HAMILTONIAN/sparse/H_local.f90:1-102
 *       H_up / H_dw          ED_HAMILTONIAN/sparse/H_up.f90:1-89, H_dw.f90:1-89
 *       H_non_local          ED_HAMILTONIAN/sparse/H_non_local.f90:4-100
 *   - spMatVec_main          ED_HAMILTONIAN_SPARSE_HxV.f90:167-227
 *   - spMatVec_mpi_main      ED_HAMILTONIAN_SPARSE_HxV.f90:230-315 (+ the DimDw split
 *                            ED_HAMILTONIAN.f90:93-105 and vector_transpose_MPI
 *                            ED_HAMILTONIAN_COMMON.f90:30-101), ranks emulated by threads
 *   - dense Hmat             ED_HAMILTONIAN_SPARSE_HxV.f90:112-148
 *   - Lanczos tridiag / eigh the consumer-side contract at ED_GF_NORMAL.f90:204-220,
 *                            :915-975 and ED_DIAG.f90:176-184.  The drivers themselves
 *                            live in the THIRD-PARTY library SciFortran (SF_SP_LINALG,
 *                            version hint "4.10.8" at drivers/cdn_bhz_2d.f90:3), which is
 *                            not vendored: the plain 3-term Lanczos recurrence is restated
 *                            from its published algorithm.
 *
 * PINNING STATUS
 *   The reference has no tests, fixtures or golden vectors, and it
 *   cannot be built in this image without writing stand-ins for SciFortran, MPI and the
 *   CMake-generated revision.inc, which the build rules forbid.  The H x V part of this
 *   oracle is therefore pinned by (tests/test_oracle_pins.py):
 *     (1) numbers the survey recorded from the reference itself (SURVEY.md 8c, App. A.5b,
 *         BASELINE.md section 2): lowest eigenvalues of the reference-built dense H for the
 *         2x2 plaquette sector (2,2) and the complex BHZ sectors (4,4), (3,5); nnz counts
 *         of H_up for C1/C2/C3 and the BHZ sector; exact Hermiticity; max|Im H| = 0.15;
 *     (2) the literature value E0 = -2.10275 t of the 4-site Hubbard ring at U = 4t;
 *     (3) an independent second-quantised (Jordan-Wigner, full Fock space) construction
 *         in numpy, sector by sector, at Ns <= 4;
 *     (4) internal consistency sparse == dense-Kronecker == mpi-emulated product.
 *   The Lanczos part is "parity unpinned" against SciFortran itself (absent); it is pinned
 *   against LAPACK on the dense H and against the Lehmann representation of G.
 */
#include <complex.h>
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef double _Complex zc;

/* ------------------------------------------------------------------ */
/* row-list sparse matrix: ED_SPARSE_MATRIX.f90:13-30                  */
/* ------------------------------------------------------------------ */
typedef struct {
  int size;
  zc *vals;
  int *cols; /* 1-based, as in the reference */
} sp_row;

typedef struct {
  int nrow, ncol;
  sp_row *row;
} sp_matrix;

static void sp_init_matrix(sp_matrix *m, int n) { /* ED_SPARSE_MATRIX.f90:127-172 */
  m->nrow = n;
  m->ncol = n;
  m->row = (sp_row *)calloc((size_t)(n > 0 ? n : 1), sizeof(sp_row));
}

static void sp_delete_matrix(sp_matrix *m) { /* ED_SPARSE_MATRIX.f90:184-236 */
  if (!m->row) return;
  for (int i = 0; i < m->nrow; i++) {
    free(m->row[i].vals);
    free(m->row[i].cols);
  }
  free(m->row);
  m->row = NULL;
  m->nrow = m->ncol = 0;
}

/* ED_SPARSE_MATRIX.f90:254-322: existing column -> sum, else append at the end. */
static void sp_insert_element(sp_matrix *m, zc value, int i, int j) {
  sp_row *r = &m->row[i - 1];
  for (int k = 0; k < r->size; k++) {
    if (r->cols[k] == j) {
      r->vals[k] += value;
      return;
    }
  }
  r->vals = (zc *)realloc(r->vals, sizeof(zc) * (size_t)(r->size + 1));
  r->cols = (int *)realloc(r->cols, sizeof(int) * (size_t)(r->size + 1));
  r->vals[r->size] = value;
  r->cols[r->size] = j;
  r->size += 1;
}

/* ------------------------------------------------------------------ */
/* sector / model state: the module globals of ED_VARS_GLOBAL +         */
/* ED_HAMILTONIAN_COMMON.f90:11-20, gathered in one struct              */
/* ------------------------------------------------------------------ */
typedef struct {
  int Nlat, Norb, Nspin, Nbath, Nimp, Ns;
  int hfmode, Jhflag;
  double Uloc[5], Ust, Jh, Jx, Jp, xmu;
  zc *impHloc;     /* (Nlat,Nlat,Nspin,Nspin,Norb,Norb)        Fortran order */
  zc *Hbath;       /* (Nlat,Nlat,Nspin,Nspin,Norb,Norb,Nbath)  Fortran order */
  double *diag_hybr; /* (Nlat,Nspin,Norb,Nbath) */
  double *bath_diag; /* (Nlat,Nspin,Norb,Nbath) */
  int nup, ndw;
  int DimUp, DimDw;
  int64_t Dim;
  int *map_up, *map_dw; /* Hs(1)%map, Hs(2)%map */
  /* MPI split, ED_HAMILTONIAN.f90:93-105 */
  int MpiRank, MpiSize, mpiQdw;
  int64_t mpiIstart, mpiIend, mpiIshift;
  /* matrices */
  zc *spH0d; /* one element per local row (rows of size 1): sparse/H_local.f90:95-100 */
  sp_matrix spH0ups, spH0dws, spH0nd;
} orc_sector;

/* ED_SETUP.f90:1019-1037 */
static int64_t binomial(int n, int k) {
  if (k < 0 || k > n) return 0;
  if (k > n - k) k = n - k;
  int64_t r = 1;
  for (int i = 1; i <= k; i++) r = r * (n - k + i) / i;
  return r;
}

/* ED_SETUP.f90:563-568 */
static int imp_state_index(const orc_sector *s, int ilat, int iorb) {
  return iorb + (ilat - 1) * s->Norb;
}
/* ED_SETUP.f90:367-375 */
static int getBathStride(const orc_sector *s, int ilat, int iorb, int ibath) {
  return s->Nlat * s->Norb + imp_state_index(s, ilat, iorb) + (ibath - 1) * s->Nlat * s->Norb;
}
/* ED_AUX_FUNX.f90:81-87 (used only by callers that fill diag_hybr) */

/* Fortran-order indexers, 1-based arguments */
static size_t ix6(const orc_sector *s, int il, int jl, int is, int js, int io, int jo) {
  size_t L = (size_t)s->Nlat, S = (size_t)s->Nspin, O = (size_t)s->Norb;
  return (size_t)(il - 1) +
         L * ((size_t)(jl - 1) + L * ((size_t)(is - 1) + S * ((size_t)(js - 1) + S * ((size_t)(io - 1) + O * (size_t)(jo - 1)))));
}
static size_t ix7(const orc_sector *s, int il, int jl, int is, int js, int io, int jo, int ib) {
  size_t L = (size_t)s->Nlat, S = (size_t)s->Nspin, O = (size_t)s->Norb;
  return ix6(s, il, jl, is, js, io, jo) + L * L * S * S * O * O * (size_t)(ib - 1);
}
static size_t ix4(const orc_sector *s, int il, int is, int io, int ib) {
  size_t L = (size_t)s->Nlat, S = (size_t)s->Nspin, O = (size_t)s->Norb;
  return (size_t)(il - 1) + L * ((size_t)(is - 1) + S * ((size_t)(io - 1) + O * (size_t)(ib - 1)));
}

/* ED_SETUP.f90:748-773: ascending integers with the right popcount */
static void build_sector_map(int Ns, int n, int *map) {
  int imap = 0;
  for (unsigned m = 0; m < (1u << Ns); m++) {
    if (__builtin_popcount(m) != n) continue;
    map[imap++] = (int)m;
  }
}

/* ED_SETUP.f90:807-819 */
static void op_c(int pos, int in, int *out, double *fsgn) {
  if (!((in >> (pos - 1)) & 1)) {
    fprintf(stderr, "C error: C_i|...0_i...>\n");
    abort();
  }
  *fsgn = 1.0;
  for (int l = 1; l <= pos - 1; l++)
    if ((in >> (l - 1)) & 1) *fsgn = -*fsgn;
  *out = in & ~(1 << (pos - 1));
}
/* ED_SETUP.f90:821-833 */
static void op_cdg(int pos, int in, int *out, double *fsgn) {
  if ((in >> (pos - 1)) & 1) {
    fprintf(stderr, "C^+ error: C^+_i|...1_i...>\n");
    abort();
  }
  *fsgn = 1.0;
  for (int l = 1; l <= pos - 1; l++)
    if ((in >> (l - 1)) & 1) *fsgn = -*fsgn;
  *out = in | (1 << (pos - 1));
}
/* ED_SETUP.f90:1044-1061: position (1-based) of value in the sorted map, 0 if absent */
static int binary_search(const int *a, int n, int value) {
  int lo = 0, hi = n - 1;
  while (lo <= hi) {
    int mid = (lo + hi) / 2;
    if (a[mid] == value) return mid + 1;
    if (a[mid] < value) lo = mid + 1;
    else hi = mid - 1;
  }
  return 0;
}

/* ------------------------------------------------------------------ */
/* ed_buildh_main: ED_HAMILTONIAN_SPARSE_HxV.f90:40-110                 */
/* ------------------------------------------------------------------ */
static void build_one_spin(orc_sector *s, sp_matrix *sp, const int *map, int dim, int spin) {
  /* sparse/H_up.f90:1-89 (spin=1) and sparse/H_dw.f90:1-89 (spin=Nspin) */
  int ib[64];
  for (int jup = 1; jup <= dim; jup++) {
    int mup = map[jup - 1];
    for (int l = 0; l < s->Ns; l++) ib[l + 1] = (mup >> l) & 1; /* bdecomp */
    int k1, k2, iup;
    double sg1, sg2;
    /* H_imp off-diagonal: H_up.f90:8-28 */
    for (int ilat = 1; ilat <= s->Nlat; ilat++)
      for (int jlat = 1; jlat <= s->Nlat; jlat++)
        for (int iorb = 1; iorb <= s->Norb; iorb++)
          for (int jorb = 1; jorb <= s->Norb; jorb++) {
            int is = imp_state_index(s, ilat, iorb);
            int js = imp_state_index(s, jlat, jorb);
            zc t = s->impHloc[ix6(s, ilat, jlat, spin, spin, iorb, jorb)];
            if (t != 0.0 && ib[js] == 1 && ib[is] == 0) {
              op_c(js, mup, &k1, &sg1);
              op_cdg(is, k1, &k2, &sg2);
              iup = binary_search(map, dim, k2);
              sp_insert_element(sp, t * sg1 * sg2, iup, jup);
            }
          }
    /* H_bath inter-orbital hops: H_up.f90:31-56 */
    for (int ibath = 1; ibath <= s->Nbath; ibath++)
      for (int ilat = 1; ilat <= s->Nlat; ilat++)
        for (int jlat = 1; jlat <= s->Nlat; jlat++)
          for (int iorb = 1; iorb <= s->Norb; iorb++)
            for (int jorb = 1; jorb <= s->Norb; jorb++) {
              int ialfa = getBathStride(s, ilat, iorb, ibath);
              int ibeta = getBathStride(s, jlat, jorb, ibath);
              zc t = s->Hbath[ix7(s, ilat, jlat, spin, spin, iorb, jorb, ibath)];
              if (t != 0.0 && ib[ibeta] == 1 && ib[ialfa] == 0) {
                op_c(ibeta, mup, &k1, &sg1);
                op_cdg(ialfa, k1, &k2, &sg2);
                iup = binary_search(map, dim, k2);
                sp_insert_element(sp, t * sg1 * sg2, iup, jup);
              }
            }
    /* H_hyb: H_up.f90:60-87 */
    for (int ilat = 1; ilat <= s->Nlat; ilat++)
      for (int iorb = 1; iorb <= s->Norb; iorb++)
        for (int ibath = 1; ibath <= s->Nbath; ibath++) {
          int ialfa = getBathStride(s, ilat, iorb, ibath);
          int is = imp_state_index(s, ilat, iorb);
          double V = s->diag_hybr[ix4(s, ilat, spin, iorb, ibath)];
          if (V != 0.0 && ib[is] == 1 && ib[ialfa] == 0) {
            op_c(is, mup, &k1, &sg1);
            op_cdg(ialfa, k1, &k2, &sg2);
            iup = binary_search(map, dim, k2);
            sp_insert_element(sp, V * sg1 * sg2, iup, jup);
          }
          if (V != 0.0 && ib[is] == 0 && ib[ialfa] == 1) {
            op_c(ialfa, mup, &k1, &sg1);
            op_cdg(is, k1, &k2, &sg2);
            iup = binary_search(map, dim, k2);
            sp_insert_element(sp, V * sg1 * sg2, iup, jup);
          }
        }
  }
}

static void build_local(orc_sector *s) {
  /* sparse/H_local.f90:1-102 */
  int Nlat = s->Nlat, Norb = s->Norb, Nspin = s->Nspin;
  double nup[16][8], ndw[16][8];
  int ibup[64], ibdw[64];
  for (int64_t i = s->mpiIstart; i <= s->mpiIend; i++) {
    int iup = (int)(i % s->DimUp);
    if (iup == 0) iup = s->DimUp;               /* ED_SETUP.f90:547-552 */
    int idw = (int)((i - 1) / s->DimUp) + 1;    /* ED_SETUP.f90:555-560 */
    int mup = s->map_up[iup - 1], mdw = s->map_dw[idw - 1];
    for (int l = 0; l < s->Ns; l++) {
      ibup[l + 1] = (mup >> l) & 1;
      ibdw[l + 1] = (mdw >> l) & 1;
    }
    for (int ilat = 1; ilat <= Nlat; ilat++)
      for (int iorb = 1; iorb <= Norb; iorb++) {
        nup[ilat][iorb] = (double)ibup[imp_state_index(s, ilat, iorb)];
        ndw[ilat][iorb] = (double)ibdw[imp_state_index(s, ilat, iorb)];
      }
    zc htmp = 0.0;
    /* :22-28 */
    for (int ilat = 1; ilat <= Nlat; ilat++)
      for (int iorb = 1; iorb <= Norb; iorb++) {
        htmp += s->impHloc[ix6(s, ilat, ilat, 1, 1, iorb, iorb)] * nup[ilat][iorb];
        htmp += s->impHloc[ix6(s, ilat, ilat, Nspin, Nspin, iorb, iorb)] * ndw[ilat][iorb];
        htmp -= s->xmu * (nup[ilat][iorb] + ndw[ilat][iorb]);
      }
    /* :35-39 */
    for (int ilat = 1; ilat <= Nlat; ilat++)
      for (int iorb = 1; iorb <= Norb; iorb++) htmp += s->Uloc[iorb - 1] * nup[ilat][iorb] * ndw[ilat][iorb];
    if (Norb > 1) {
      /* :44-50 */
      for (int ilat = 1; ilat <= Nlat; ilat++)
        for (int iorb = 1; iorb <= Norb; iorb++)
          for (int jorb = iorb + 1; jorb <= Norb; jorb++)
            htmp += s->Ust * (nup[ilat][iorb] * ndw[ilat][jorb] + nup[ilat][jorb] * ndw[ilat][iorb]);
      /* :54-60 */
      for (int ilat = 1; ilat <= Nlat; ilat++)
        for (int iorb = 1; iorb <= Norb; iorb++)
          for (int jorb = iorb + 1; jorb <= Norb; jorb++)
            htmp += (s->Ust - s->Jh) * (nup[ilat][iorb] * nup[ilat][jorb] + ndw[ilat][iorb] * ndw[ilat][jorb]);
    }
    /* :64-80 */
    if (s->hfmode) {
      for (int ilat = 1; ilat <= Nlat; ilat++)
        for (int iorb = 1; iorb <= Norb; iorb++)
          htmp = htmp - 0.5 * s->Uloc[iorb - 1] * (nup[ilat][iorb] + ndw[ilat][iorb]) + 0.25 * s->Uloc[iorb - 1]; /* (htmp - a) + b, as :67 */
      if (Norb > 1) {
        for (int ilat = 1; ilat <= Nlat; ilat++)
          for (int iorb = 1; iorb <= Norb; iorb++)
            for (int jorb = iorb + 1; jorb <= Norb; jorb++) {
              double nn = nup[ilat][iorb] + ndw[ilat][iorb] + nup[ilat][jorb] + ndw[ilat][jorb];
              htmp = htmp - 0.5 * s->Ust * nn + 0.25 * s->Ust; /* left to right, as :74-75 */
              htmp = htmp - 0.5 * (s->Ust - s->Jh) * nn + 0.25 * (s->Ust - s->Jh);
            }
      }
    }
    /* :85-93 */
    for (int ilat = 1; ilat <= Nlat; ilat++)
      for (int iorb = 1; iorb <= Norb; iorb++)
        for (int ibath = 1; ibath <= s->Nbath; ibath++) {
          int ialfa = getBathStride(s, ilat, iorb, ibath);
          htmp += s->bath_diag[ix4(s, ilat, 1, iorb, ibath)] * ibup[ialfa];
          htmp += s->bath_diag[ix4(s, ilat, Nspin, iorb, ibath)] * ibdw[ialfa];
        }
    s->spH0d[i - s->mpiIshift - 1] = htmp; /* sp_insert_element(spH0d,htmp,i,i) */
  }
}

static void build_non_local(orc_sector *s) {
  /* sparse/H_non_local.f90:4-100 ; rows are local (i - Ishift), columns global */
  int Nlat = s->Nlat, Norb = s->Norb;
  double nup[16][8], ndw[16][8];
  for (int64_t i = s->mpiIstart; i <= s->mpiIend; i++) {
    int iup = (int)(i % s->DimUp);
    if (iup == 0) iup = s->DimUp;
    int idw = (int)((i - 1) / s->DimUp) + 1;
    int mup = s->map_up[iup - 1], mdw = s->map_dw[idw - 1];
    for (int ilat = 1; ilat <= Nlat; ilat++)
      for (int iorb = 1; iorb <= Norb; iorb++) {
        nup[ilat][iorb] = (double)((mup >> (imp_state_index(s, ilat, iorb) - 1)) & 1);
        ndw[ilat][iorb] = (double)((mdw >> (imp_state_index(s, ilat, iorb) - 1)) & 1);
      }
    int k1, k2, k3, k4, jup, jdw;
    double sg1, sg2, sg3, sg4;
    if (s->Jx != 0.0) { /* :26-60 */
      for (int ilat = 1; ilat <= Nlat; ilat++)
        for (int iorb = 1; iorb <= Norb; iorb++)
          for (int jorb = 1; jorb <= Norb; jorb++) {
            int is = imp_state_index(s, ilat, iorb), js = imp_state_index(s, ilat, jorb);
            if (is != js && nup[ilat][jorb] == 1 && ndw[ilat][iorb] == 1 && ndw[ilat][jorb] == 0 && nup[ilat][iorb] == 0) {
              op_c(is, mdw, &k1, &sg1);
              op_cdg(js, k1, &k2, &sg2);
              jdw = binary_search(s->map_dw, s->DimDw, k2);
              op_c(js, mup, &k3, &sg3);
              op_cdg(is, k3, &k4, &sg4);
              jup = binary_search(s->map_up, s->DimUp, k4);
              int64_t j = jup + (int64_t)(jdw - 1) * s->DimUp;
              sp_insert_element(&s->spH0nd, s->Jx * sg1 * sg2 * sg3 * sg4, (int)(i - s->mpiIshift), (int)j);
            }
          }
    }
    if (s->Jp != 0.0) { /* :65-98 */
      for (int ilat = 1; ilat <= Nlat; ilat++)
        for (int iorb = 1; iorb <= Norb; iorb++)
          for (int jorb = 1; jorb <= Norb; jorb++) {
            int is = imp_state_index(s, ilat, iorb), js = imp_state_index(s, ilat, jorb);
            if (nup[ilat][jorb] == 1 && ndw[ilat][jorb] == 1 && ndw[ilat][iorb] == 0 && nup[ilat][iorb] == 0) {
              op_c(js, mdw, &k1, &sg1);
              op_cdg(is, k1, &k2, &sg2);
              jdw = binary_search(s->map_dw, s->DimDw, k2);
              op_c(js, mup, &k3, &sg3);
              op_cdg(is, k3, &k4, &sg4);
              jup = binary_search(s->map_up, s->DimUp, k4);
              int64_t j = jup + (int64_t)(jdw - 1) * s->DimUp;
              sp_insert_element(&s->spH0nd, s->Jp * sg1 * sg2 * sg3 * sg4, (int)(i - s->mpiIshift), (int)j);
            }
          }
    }
  }
}

/* ------------------------------------------------------------------ */
/* public API (ctypes)                                                  */
/* ------------------------------------------------------------------ */

/* build_Hv_sector + ed_buildh_main.  Complex arrays are passed as interleaved (re,im)
 * doubles in the reference's Fortran array order.  mpi_size=1 -> serial (MpiStatus=F). */
orc_sector *orc_open(int Nlat, int Norb, int Nspin, int Nbath, int nup, int ndw, const double *Uloc5, double Ust, double Jh,
                     double Jx, double Jp, double xmu, int hfmode, const double *impHloc_ri, const double *Hbath_ri,
                     const double *Vbath, int mpi_rank, int mpi_size) {
  orc_sector *s = (orc_sector *)calloc(1, sizeof(orc_sector));
  s->Nlat = Nlat; s->Norb = Norb; s->Nspin = Nspin; s->Nbath = Nbath;
  s->Nimp = Nlat * Norb;            /* ED_SETUP.f90:113 */
  s->Ns = s->Nimp * (Nbath + 1);    /* ED_SETUP.f90:114 */
  if (s->Ns > 30 || Nlat > 15 || Norb > 7) { free(s); return NULL; }
  s->hfmode = hfmode;
  for (int i = 0; i < 5; i++) s->Uloc[i] = Uloc5[i];
  s->Ust = Ust; s->Jh = Jh; s->Jx = Jx; s->Jp = Jp; s->xmu = xmu;
  s->Jhflag = (Norb > 1) && (Jx != 0.0 || Jp != 0.0); /* ED_SETUP.f90:200-201 */
  size_t n6 = (size_t)Nlat * Nlat * Nspin * Nspin * Norb * Norb;
  s->impHloc = (zc *)malloc(sizeof(zc) * n6);
  for (size_t k = 0; k < n6; k++) s->impHloc[k] = impHloc_ri[2 * k] + I * impHloc_ri[2 * k + 1];
  size_t n7 = n6 * (size_t)(Nbath > 0 ? Nbath : 1), n4 = (size_t)Nlat * Nspin * Norb * (size_t)(Nbath > 0 ? Nbath : 1);
  s->Hbath = (zc *)calloc(n7, sizeof(zc));
  s->diag_hybr = (double *)calloc(n4, sizeof(double));
  s->bath_diag = (double *)calloc(n4, sizeof(double));
  for (size_t k = 0; k < n6 * (size_t)Nbath; k++) s->Hbath[k] = Hbath_ri[2 * k] + I * Hbath_ri[2 * k + 1];
  /* ED_HAMILTONIAN_SPARSE_HxV.f90:62-76 */
  for (int ib = 1; ib <= Nbath; ib++)
    for (int il = 1; il <= Nlat; il++)
      for (int is = 1; is <= Nspin; is++)
        for (int io = 1; io <= Norb; io++) {
          s->diag_hybr[ix4(s, il, is, io, ib)] = Vbath[ix4(s, il, is, io, ib)];
          s->bath_diag[ix4(s, il, is, io, ib)] = creal(s->Hbath[ix7(s, il, il, is, is, io, io, ib)]);
        }
  s->nup = nup; s->ndw = ndw;
  s->DimUp = (int)binomial(s->Ns, nup);
  s->DimDw = (int)binomial(s->Ns, ndw);
  s->Dim = (int64_t)s->DimUp * s->DimDw;
  s->map_up = (int *)malloc(sizeof(int) * (size_t)s->DimUp);
  s->map_dw = (int *)malloc(sizeof(int) * (size_t)s->DimDw);
  build_sector_map(s->Ns, nup, s->map_up);
  build_sector_map(s->Ns, ndw, s->map_dw);
  /* Dw split: ED_HAMILTONIAN.f90:93-105 */
  s->MpiRank = mpi_rank; s->MpiSize = mpi_size;
  int q = s->DimDw / mpi_size, rdw = s->DimDw % mpi_size;
  if (mpi_rank < s->DimDw % mpi_size) { rdw = 0; q += 1; }
  s->mpiQdw = q;
  int64_t mpiQ = (int64_t)s->DimUp * q, mpiR = (int64_t)s->DimUp * rdw;
  s->mpiIstart = 1 + mpi_rank * mpiQ + mpiR;
  s->mpiIend = (mpi_rank + 1) * mpiQ + mpiR;
  s->mpiIshift = mpi_rank * mpiQ + mpiR;
  /* matrices */
  s->spH0d = (zc *)calloc((size_t)(mpiQ > 0 ? mpiQ : 1), sizeof(zc));
  sp_init_matrix(&s->spH0ups, s->DimUp);
  sp_init_matrix(&s->spH0dws, s->DimDw);
  build_local(s);
  if (s->Jhflag) {
    s->spH0nd.nrow = (int)mpiQ; s->spH0nd.ncol = (int)s->Dim;
    s->spH0nd.row = (sp_row *)calloc((size_t)(mpiQ > 0 ? mpiQ : 1), sizeof(sp_row));
    build_non_local(s);
  }
  build_one_spin(s, &s->spH0ups, s->map_up, s->DimUp, 1);
  build_one_spin(s, &s->spH0dws, s->map_dw, s->DimDw, Nspin);
  return s;
}

/* delete_Hv_sector: ED_HAMILTONIAN.f90:149-190 */
void orc_close(orc_sector *s) {
  if (!s) return;
  sp_delete_matrix(&s->spH0ups);
  sp_delete_matrix(&s->spH0dws);
  sp_delete_matrix(&s->spH0nd);
  free(s->spH0d); free(s->map_up); free(s->map_dw);
  free(s->impHloc); free(s->Hbath); free(s->diag_hybr); free(s->bath_diag);
  free(s);
}

int orc_dim_up(const orc_sector *s) { return s->DimUp; }
int orc_dim_dw(const orc_sector *s) { return s->DimDw; }
int64_t orc_dim(const orc_sector *s) { return s->Dim; }
int orc_qdw(const orc_sector *s) { return s->mpiQdw; }
int64_t orc_ishift(const orc_sector *s) { return s->mpiIshift; }
/* vecDim_Hv_sector: ED_HAMILTONIAN.f90:197-221 */
int64_t orc_vecdim(const orc_sector *s) { return (int64_t)s->DimUp * s->mpiQdw; }
const int *orc_map_up(const orc_sector *s) { return s->map_up; }
const int *orc_map_dw(const orc_sector *s) { return s->map_dw; }
const double *orc_diag_ri(const orc_sector *s) { return (const double *)s->spH0d; }

static const sp_matrix *pick(const orc_sector *s, int which) {
  return which == 0 ? &s->spH0ups : which == 1 ? &s->spH0dws : &s->spH0nd;
}
int64_t orc_nnz(const orc_sector *s, int which) {
  const sp_matrix *m = pick(s, which);
  int64_t n = 0;
  for (int i = 0; i < m->nrow; i++) n += m->row[i].size;
  return n;
}
/* flat CSR dump in row-list (insertion) order; cols stay 1-based */
void orc_dump_csr(const orc_sector *s, int which, int64_t *rowptr, int *cols, double *vals_ri) {
  const sp_matrix *m = pick(s, which);
  int64_t p = 0;
  for (int i = 0; i < m->nrow; i++) {
    rowptr[i] = p;
    for (int k = 0; k < m->row[i].size; k++, p++) {
      cols[p] = m->row[i].cols[k];
      vals_ri[2 * p] = creal(m->row[i].vals[k]);
      vals_ri[2 * p + 1] = cimag(m->row[i].vals[k]);
    }
  }
  rowptr[m->nrow] = p;
}

/* spMatVec_main: ED_HAMILTONIAN_SPARSE_HxV.f90:167-227 (serial; needs mpi_size==1) */
int orc_spmatvec_main(const orc_sector *s, int64_t Nloc, const double *v_ri, double *Hv_ri) {
  if (s->MpiSize != 1 || Nloc != s->Dim) return 1;
  const zc *v = (const zc *)v_ri;
  zc *Hv = (zc *)Hv_ri;
  int DimUp = s->DimUp, DimDw = s->DimDw;
  for (int64_t i = 0; i < Nloc; i++) Hv[i] = 0.0;
  for (int64_t i = 0; i < Nloc; i++) Hv[i] += s->spH0d[i] * v[i]; /* :178-182 */
  for (int iup = 1; iup <= DimUp; iup++)                          /* :185-198 */
    for (int idw = 1; idw <= DimDw; idw++) {
      int64_t i = iup + (int64_t)(idw - 1) * DimUp;
      const sp_row *r = &s->spH0dws.row[idw - 1];
      for (int jj = 0; jj < r->size; jj++) {
        int64_t j = iup + (int64_t)(r->cols[jj] - 1) * DimUp;
        Hv[i - 1] += r->vals[jj] * v[j - 1];
      }
    }
  for (int idw = 1; idw <= DimDw; idw++)                          /* :201-214 */
    for (int iup = 1; iup <= DimUp; iup++) {
      int64_t i = iup + (int64_t)(idw - 1) * DimUp;
      const sp_row *r = &s->spH0ups.row[iup - 1];
      for (int jj = 0; jj < r->size; jj++) {
        int64_t j = r->cols[jj] + (int64_t)(idw - 1) * DimUp;
        Hv[i - 1] += r->vals[jj] * v[j - 1];
      }
    }
  if (s->Jhflag)                                                   /* :217-225 */
    for (int64_t i = 0; i < Nloc; i++) {
      const sp_row *r = &s->spH0nd.row[i];
      for (int jj = 0; jj < r->size; jj++) Hv[i] += r->vals[jj] * v[r->cols[jj] - 1];
    }
  return 0;
}

/* Dense sector Hamiltonian, column-major Dim x Dim:
 * diag + kron(H_dw, 1_up) + kron(1_dw, H_up) [+ H_nd]   (:112-148) */
int orc_dense(const orc_sector *s, double *H_ri) {
  if (s->MpiSize != 1) return 1;
  int64_t D = s->Dim;
  zc *H = (zc *)H_ri;
  memset(H, 0, sizeof(zc) * (size_t)D * (size_t)D);
  for (int64_t i = 0; i < D; i++) H[i + i * D] += s->spH0d[i];
  for (int idw = 0; idw < s->DimDw; idw++) {
    const sp_row *r = &s->spH0dws.row[idw];
    for (int jj = 0; jj < r->size; jj++)
      for (int iup = 0; iup < s->DimUp; iup++) {
        int64_t i = iup + (int64_t)idw * s->DimUp, j = iup + (int64_t)(r->cols[jj] - 1) * s->DimUp;
        H[i + j * D] += r->vals[jj];
      }
  }
  for (int iup = 0; iup < s->DimUp; iup++) {
    const sp_row *r = &s->spH0ups.row[iup];
    for (int jj = 0; jj < r->size; jj++)
      for (int idw = 0; idw < s->DimDw; idw++) {
        int64_t i = iup + (int64_t)idw * s->DimUp, j = (r->cols[jj] - 1) + (int64_t)idw * s->DimUp;
        H[i + j * D] += r->vals[jj];
      }
  }
  if (s->Jhflag)
    for (int64_t i = 0; i < D; i++) {
      const sp_row *r = &s->spH0nd.row[i];
      for (int jj = 0; jj < r->size; jj++) H[i + (int64_t)(r->cols[jj] - 1) * D] += r->vals[jj];
    }
  return 0;
}

/* ------------------------------------------------------------------ */
/* spMatVec_mpi_main, ranks emulated by threads in shared memory.       */
/* One orc_sector per rank (opened with mpi_rank=r, mpi_size=P); the    */
/* "communicator" is the array of sectors.  The two vector_transpose_MPI*/
/* calls (ED_HAMILTONIAN_COMMON.f90:30-94) become direct strided copies */
/* between the ranks' slabs, separated by barriers.                     */
/* ------------------------------------------------------------------ */
typedef struct {
  int P, rank;
  orc_sector **sec;
  const zc *v;   /* full vector, rank r reads only its slab  */
  zc *Hv;        /* full output, rank r writes only its slab */
  zc *vt, *Hvt;  /* transposed global buffers [DimDw x DimUp] (column = iup) */
  pthread_barrier_t *bar;
} mpi_task;

static void up_split(int DimUp, int P, int r, int *q, int *start) {
  /* mpiQup: ED_HAMILTONIAN_SPARSE_HxV.f90:274-275 (same rule as the Dw split) */
  int qq = DimUp / P, rem = DimUp % P;
  *q = qq + (r < rem ? 1 : 0);
  *start = r * qq + (r < rem ? r : rem);
}

static void *mpi_rank_body(void *arg) {
  mpi_task *t = (mpi_task *)arg;
  const orc_sector *s = t->sec[t->rank];
  int DimUp = s->DimUp, DimDw = s->DimDw, Qdw = s->mpiQdw;
  int64_t sh = s->mpiIshift;
  const zc *v = t->v + sh;
  zc *Hv = t->Hv + sh;
  int64_t Nloc = (int64_t)DimUp * Qdw;
  int dw0 = (int)(sh / DimUp);
  /* :250-255 diagonal */
  for (int64_t i = 0; i < Nloc; i++) Hv[i] = s->spH0d[i] * v[i];
  /* :259-270 up hops, contiguous */
  for (int idw = 0; idw < Qdw; idw++)
    for (int iup = 0; iup < DimUp; iup++) {
      const sp_row *r = &s->spH0ups.row[iup];
      zc acc = 0.0;
      for (int jj = 0; jj < r->size; jj++) acc += r->vals[jj] * v[(r->cols[jj] - 1) + (int64_t)idw * DimUp];
      Hv[iup + (int64_t)idw * DimUp] += acc;
    }
  /* :279 transpose #1: my slab v(DimUp, Qdw) -> vt(DimDw, iup) for all iup */
  for (int idw = 0; idw < Qdw; idw++)
    for (int iup = 0; iup < DimUp; iup++) t->vt[(int64_t)(dw0 + idw) + (int64_t)iup * DimDw] = v[iup + (int64_t)idw * DimUp];
  pthread_barrier_wait(t->bar);
  /* :281-292 dw hops on my DimDw x mpiQup transposed slab */
  int Qup, up0;
  up_split(DimUp, t->P, t->rank, &Qup, &up0);
  for (int iu = 0; iu < Qup; iu++) {
    const zc *col = t->vt + (int64_t)(up0 + iu) * DimDw;
    zc *out = t->Hvt + (int64_t)(up0 + iu) * DimDw;
    for (int idw = 0; idw < DimDw; idw++) {
      const sp_row *r = &s->spH0dws.row[idw];
      zc acc = 0.0;
      for (int jj = 0; jj < r->size; jj++) acc += r->vals[jj] * col[r->cols[jj] - 1];
      out[idw] = acc;
    }
  }
  pthread_barrier_wait(t->bar);
  /* :294-295 transpose #2 and add */
  for (int idw = 0; idw < Qdw; idw++)
    for (int iup = 0; iup < DimUp; iup++) Hv[iup + (int64_t)idw * DimUp] += t->Hvt[(int64_t)(dw0 + idw) + (int64_t)iup * DimDw];
  /* :300-313 non-local block on the allgathered vector (= t->v in shared memory) */
  if (s->Jhflag)
    for (int64_t i = 0; i < Nloc; i++) {
      const sp_row *r = &s->spH0nd.row[i];
      for (int jj = 0; jj < r->size; jj++) Hv[i] += r->vals[jj] * t->v[r->cols[jj] - 1];
    }
  return NULL;
}

/* work = caller-provided scratch of 2*Dim complex (vt, Hvt), so repeated timed calls do
 * not pay allocation (the reference allocates per call, :277-296; we do not time that). */
int orc_spmatvec_mpi_main(orc_sector **sec, int P, const double *v_ri, double *Hv_ri, double *work_ri) {
  if (P < 1 || P > 256) return 1;
  int64_t D = sec[0]->Dim;
  pthread_barrier_t bar;
  pthread_barrier_init(&bar, NULL, (unsigned)P);
  pthread_t th[256];
  mpi_task task[256];
  for (int r = 0; r < P; r++) {
    task[r].P = P; task[r].rank = r; task[r].sec = sec;
    task[r].v = (const zc *)v_ri; task[r].Hv = (zc *)Hv_ri;
    task[r].vt = (zc *)work_ri; task[r].Hvt = (zc *)work_ri + D;
    task[r].bar = &bar;
  }
  for (int r = 1; r < P; r++) pthread_create(&th[r], NULL, mpi_rank_body, &task[r]);
  mpi_rank_body(&task[0]);
  for (int r = 1; r < P; r++) pthread_join(th[r], NULL);
  pthread_barrier_destroy(&bar);
  return 0;
}

/* ------------------------------------------------------------------ */
/* Plain Lanczos (SciFortran sp_lanc_tridiag / sp_lanc_eigh contract).  */
/* alanc(k) = <q_k|H|q_k>, blanc(k+1) = ||H q_k - a_k q_k - b_k q_{k-1}||,*/
/* blanc(1) unused (ED_GF_NORMAL.f90:949-951).  vin is normalised by the */
/* caller (ED_GF_NORMAL.f90:197-199).  Returns the number of steps done. */
/* ------------------------------------------------------------------ */
int orc_lanc_tridiag(const orc_sector *s, const double *vin_ri, int nlanc, double *alanc, double *blanc, double threshold) {
  int64_t D = s->Dim;
  zc *q = (zc *)malloc(sizeof(zc) * (size_t)D), *qm = (zc *)calloc((size_t)D, sizeof(zc)), *w = (zc *)malloc(sizeof(zc) * (size_t)D);
  memcpy(q, vin_ri, sizeof(zc) * (size_t)D);
  double nrm = 0.0;
  for (int64_t i = 0; i < D; i++) nrm += creal(q[i]) * creal(q[i]) + cimag(q[i]) * cimag(q[i]);
  nrm = sqrt(nrm);
  for (int64_t i = 0; i < D; i++) q[i] /= nrm;
  double beta = 0.0;
  int k;
  for (k = 0; k < nlanc; k++) {
    orc_spmatvec_main(s, D, (const double *)q, (double *)w);
    double a = 0.0;
    for (int64_t i = 0; i < D; i++) {
      w[i] -= beta * qm[i];
      a += creal(conj(q[i]) * w[i]);
    }
    double b2 = 0.0;
    for (int64_t i = 0; i < D; i++) {
      w[i] -= a * q[i];
      b2 += creal(w[i]) * creal(w[i]) + cimag(w[i]) * cimag(w[i]);
    }
    alanc[k] = a;
    beta = sqrt(b2);
    if (k + 1 < nlanc) blanc[k + 1] = beta;
    if (fabs(beta) < threshold) { k++; break; }
    for (int64_t i = 0; i < D; i++) {
      qm[i] = q[i];
      q[i] = w[i] / beta;
    }
  }
  free(q); free(qm); free(w);
  return k;
}
