/*
 * hxv.h -- C-ABI of the MI355X-native sector Hamiltonian x vector engine.
 *
 * This is the drop-in boundary for ONE path of QcmPlab/CDMFT-LANC-ED: the procedure
 * pointer  spHtimesV_p  (abstract interface cc_sparse_HxV, ED_VARS_GLOBAL.f90:72-78,146)
 * and the routines that open/close the sector it acts on (ED_HAMILTONIAN.f90:39-221).
 * Plain pointers and sizes only; no C++/torch types.  Every entry returns 0 on success
 * and a non-zero hxv_status otherwise (the reference's convention is `stop "..."`,
 * e.g. ED_HAMILTONIAN_SPARSE_HxV.f90:57,247; the Fortran glue turns non-zero into stop).
 *
 * Vector layout (identical to the reference): element (iup,idw), 0-based, lives at
 *   i = iup + idw*DimUp            (ED_HAMILTONIAN/sparse/H_local.f90:2-3)
 * as complex(8) = two doubles (re,im).  A rank of an nranks-way split owns the contiguous
 * columns idw in [dw0, dw0+qdw), qdw = DimDw/nranks (+1 for rank < mod(DimDw,nranks))
 * (ED_HAMILTONIAN.f90:93-105), i.e. qdw*DimUp contiguous elements = vecDim_Hv_sector.
 */
#ifndef HXV_H
#define HXV_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hxv_handle hxv_handle;

enum hxv_status {
  HXV_OK = 0,
  HXV_ERR_ARG = 1,        /* bad argument / inconsistent sizes                          */
  HXV_ERR_HIP = 2,        /* a HIP runtime call failed (no device, OOM, launch failure) */
  HXV_ERR_STATE = 3,      /* handle not in the right state                              */
  HXV_ERR_UNSUPPORTED = 4 /* valid input the engine does not implement                  */
};

/* Operator inputs = the reference's module globals visible at bind time.
 * Complex arrays are interleaved (re,im) doubles in the reference's Fortran array order, so
 * the Fortran glue passes c_loc() of the reference arrays themselves.                      */
typedef struct {
  int32_t nlat, norb, nspin, nbath; /* ED_INPUT_VARS.f90:13-16                            */
  int32_t hfmode;                   /* ED_INPUT_VARS.f90:164 (logical -> 0/1)             */
  int32_t reserved;
  double uloc[5];                   /* ED_INPUT_VARS.f90:129                              */
  double ust, jh, jx, jp, xmu;      /* ED_INPUT_VARS.f90:130-135                          */
  const double *imphloc; /* complex (Nlat,Nlat,Nspin,Nspin,Norb,Norb)        ED_VARS_GLOBAL.f90:119 */
  const double *hbath;   /* complex (Nlat,Nlat,Nspin,Nspin,Norb,Norb,Nbath)  = Hbath_build(lambda_ib),
                            ED_HAMILTONIAN_SPARSE_HxV.f90:65; may be NULL if nbath==0      */
  const double *vbath;   /* real (Nlat,Nspin,Norb,Nbath) = diag_hybr, ED_HAMILTONIAN_SPARSE_HxV.f90:70 */
} hxv_model;

/* ---- open / close a sector -------------------------------------------------------------
 * Replaces build_Hv_sector(isector) (ED_HAMILTONIAN.f90:39-143) + ed_buildh_main
 * (ED_HAMILTONIAN_SPARSE_HxV.f90:40-110): builds the sector maps, the one-spin hopping
 * tables and the separable diagonal on the host, uploads them to HIP device `device`.
 * (nup,ndw) = get_Nup/get_Ndw(isector) (ED_SETUP.f90:477-500). rank/nranks = the DimDw
 * split of ED_HAMILTONIAN.f90:93-105 (nranks=1: serial, MpiStatus=F).  With Norb>1 and Jx or
 * Jp != 0 (Jhflag, ED_SETUP.f90:200-201) the spin-exchange / pair-hopping block spH0nd
 * (sparse/H_non_local.f90:4-100) is applied on the fly, inside the product's second pass (option "fold_nd" = 0: as a third
 * pass over Hv).                                                                         */
int hxv_create_from_model(const hxv_model *model, int32_t nup, int32_t ndw, int32_t rank, int32_t nranks, int32_t device,
                          hxv_handle **out);

/* Same, from the reference's own stored matrices (spH0ups(1), spH0dws(1), spH0d of
 * ED_VARS_GLOBAL.f90:142-144) flattened to CSR: rowptr[n+1] (0-based offsets), cols (1-based,
 * as stored by sp_insert_element ED_SPARSE_MATRIX.f90:254-322), vals interleaved complex.
 * diag = the local rows of spH0d (qdw*DimUp complex values, one per row).  A split sector (nranks > 1) takes the exchange chosen
 * by hxv_set_exchange_default like a sector opened from a model.                         */
int hxv_create_from_csr(int32_t dimup, int32_t dimdw, const int64_t *up_rowptr, const int32_t *up_cols, const double *up_vals,
                        const int64_t *dw_rowptr, const int32_t *dw_cols, const double *dw_vals, const double *diag,
                        int32_t rank, int32_t nranks, int32_t device, hxv_handle **out);

/* spH0nd of a from_csr handle (ED_VARS_GLOBAL.f90:145; built by sparse/H_non_local.f90:23-98 when Jhflag, added to Hv at
 * ED_HAMILTONIAN_SPARSE_HxV.f90:217-225 serial / :298-312 MPI): the LOCAL rows (vecDim of them) with GLOBAL 1-based column indices
 * i = iup + (idw-1)*DimUp, rowptr[vecDim+1] 0-based offsets, vals interleaved complex.  Applied as its own pass over Hv after the
 * product, from the gathered vector (all-gather exchange only).  Once per handle; not on handles opened from a model with
 * Jx / Jp (those build the block themselves).  Dim < 2^31 (the reference's column type).
 * HXV_ERR_STATE on any handle not opened with hxv_create_from_csr (a model handle's rows may be in a device row order).    */
int hxv_set_nonlocal_csr(hxv_handle *h, const int64_t *rowptr, const int32_t *cols, const double *vals);

/* delete_Hv_sector (ED_HAMILTONIAN.f90:149-190). NULL is a no-op. */
int hxv_destroy(hxv_handle *h);

/* vecDim_Hv_sector (ED_HAMILTONIAN.f90:197-221): local vector length DimUp*qdw. */
int64_t hxv_vecdim(const hxv_handle *h);
/* DimUp, DimDw, Dim, mpiQdw, mpiIshift (ED_HAMILTONIAN.f90:58-60,93-105); any out may be NULL */
int hxv_dims(const hxv_handle *h, int32_t *dimup, int32_t *dimdw, int64_t *dim, int32_t *qdw, int64_t *ishift);

/* ---- the product -----------------------------------------------------------------------
 * spHtimesV_p(Nloc,v,Hv) with HOST arrays (cc_sparse_HxV, ED_VARS_GLOBAL.f90:72-78): v, Hv = this rank's slab of
 * vecDim_Hv_sector elements; Hv is overwritten (ED_HAMILTONIAN_SPARSE_HxV.f90:175,250); synchronous.  Serial sector
 * (nranks==1) = spMatVec_main; split sector (nranks>1) = spMatVec_MPI_main: the re-assembly the reference does with two
 * MPI transposes inside the product (ED_HAMILTONIAN_SPARSE_HxV.f90:272-296) is done here by the engine itself -- one
 * ncclAllGather of the slabs over xGMI -- once the handles share a communicator (hxv_comm_init below).
 * Pays two PCIe copies of the slab per call.                                                            */
int hxv_apply_host(hxv_handle *h, int64_t nloc, const void *v, void *hv);
/* The two PCIe copies ARE this call's cost (C3: 2 x 2.65 GB; the kernels between them take 4 ms): bench.py reports it as config.apply_host next
 * to the floor the box's own H2D / D2H rates give.  Host arrays that are page-locked move by DMA at the link's rate; a host program that keeps
 * passing the same work arrays (ED_DIAG's Lanczos vectors) registers them ONCE (hipHostRegister, ~0.1 s per GB) and unregisters them before it
 * frees them.  Registering an array that is registered already is not an error.                                                          */
int hxv_host_register(void *ptr, int64_t bytes);
int hxv_host_unregister(void *ptr);

/* ---- slab exchange of a split sector (MpiStatus=T side of the boundary) -------------------------------------------
 * One RCCL communicator over the nranks handles of a sector (one process per GPU).  Rank 0 draws an id, the host program
 * broadcasts its HXV_COMM_ID_BYTES bytes by its own means (the reference: MPI_Bcast over MpiComm), every rank calls
 * hxv_comm_init (collective).  Afterwards hxv_apply_host, hxv_apply_device_slab and the device Lanczos drivers work on
 * split sectors: the product all-gathers the slabs (equal counts, all-gather layout of hxv_apply_device) on the stream it
 * runs on, the drivers' dot products are ncclAllReduce sums.  hxv_destroy unbinds the handle from the communicator (below).
 * RCCL is loaded at the first of these calls (dlopen), not at link time.                                            */
#define HXV_COMM_ID_BYTES 128
int hxv_comm_unique_id(void *id128);
int hxv_comm_init(hxv_handle *h, const void *id128);
int hxv_comm_free(hxv_handle *h);
/* ONE communicator per process, not per sector.  The reference sets MpiComm once per solve (ED_VARS_GLOBAL.f90:365-380) and derives a
 * sub-communicator only for sectors with DimDw < MpiSize (ED_HAMILTONIAN.f90:63-89), while its callers open 289 sectors per ED_DIAG sweep
 * (ED_DIAG.f90:142-190) and 56 per Green's-function stage (ED_GF_NORMAL.f90:208-222).  hxv_comm_init therefore builds a communicator
 * (ncclCommInitRank, a collective that costs far more than opening a sector) only the FIRST time it sees a (RCCL library, nranks, rank, device);
 * every later call with the same key binds the handle to that communicator and does not consume the id it is given (the host may keep
 * drawing and broadcasting ids -- 128 bytes -- or pass the first one again; every rank takes the same branch because every rank has made the
 * same calls).  A sector with DimDw < nranks is opened by the first DimDw ranks with nranks' = DimDw: another key, built once as well.
 * hxv_destroy / hxv_comm_free unbind; the communicators live until hxv_comm_cache_clear (every rank, at the same point of the program: the
 * end of a solve) or the end of the process.  A communicator that was aborted (hxv_comm_abort) or failed a collective leaves the cache: the
 * next hxv_comm_init builds a new one from its id.  Environment HXV_COMM_CACHE=0: one communicator per handle, destroyed with it.
 * hxv_comm_cache_stats: communicators cached now, ncclCommInitRank calls made so far, hxv_comm_init calls served without one (any out NULL). */
int hxv_comm_cache_stats(int64_t *entries, int64_t *inits, int64_t *reuses);
int hxv_comm_cache_clear(int64_t *destroyed);
/* A rank has failed OUTSIDE the library (its host thread / process raised before its next collective): wake this handle's rank instead of
 * leaving it inside a collective waiting for the lost peer.  RCCL communicators: ncclCommAbort -- callable from another host thread while
 * the handle's own thread blocks in a collective; that collective returns an error, the communicator is gone (later calls report a missing
 * communicator; hxv_comm_free / hxv_destroy still clean up).  Thread-rank groups: same as hxv_comm_local_abort.  HXV_ERR_UNSUPPORTED when
 * the RCCL library in use exports no ncclCommAbort.                                                                                */
int hxv_comm_abort(hxv_handle *h);
/* The file the RCCL entry points of this handle's communicator were resolved from (dladdr; "" without a communicator): which librccl a
 * multi-GPU run actually used, next to the one torch.distributed loaded.                                                          */
const char *hxv_comm_library(const hxv_handle *h);
/* STATUS of N>1 through RCCL: no round of this project has had more than one GPU, and RCCL refuses two ranks on one device, so
 * librccl itself has only ever run with ONE rank.  Everything around it -- slab copies, uneven splits, halo lists and
 * offsets, the drivers' all-reduces, the collective error agreement -- is executed with several ranks by the second
 * transport below, which shares that code; the RCCL call sites themselves (counts, offsets and pointers of the grouped
 * ncclSend / ncclRecv, the in-place ncclAllGather, the ncclMax agreement) run with 2-4 ranks against a TEST double of RCCL's ten entry
 * points (tests/rccl_double: one for thread ranks of one process, one for separate processes on one GPU): the environment variable HXV_RCCL_LIB, read by hxv_comm_unique_id /
 * hxv_comm_init, names the library to load instead of the system's librccl (a communicator keeps the library it was made with).
 * THREAD RANKS: the nranks handles of a sector live in ONE process, one host thread per rank (same GPU or different GPUs of
 * the node); slabs travel by device-to-device copies ordered with HIP events, scalars through host memory.  Create the group
 * once, then every rank's thread calls hxv_comm_init_local (collective: it returns when all nranks have joined); from then on
 * hxv_apply_host / hxv_apply_device_slab / the device drivers behave exactly as with hxv_comm_init, each called from its
 * rank's thread.  hxv_comm_free / hxv_destroy leave the group; destroy it afterwards.
 * A rank that drops out must not leave its peers waiting: a collective of the group gives up with HXV_ERR_STATE when a peer has not
 * arrived within HXV_LOCAL_TIMEOUT_S seconds (environment, default 300; read by hxv_comm_local_create), or at once after
 * hxv_comm_local_abort(group) -- what the host program calls when one rank's thread fails outside the library.  A broken group stays
 * broken: free the handles, destroy it, create a new one.  A HIP error inside a collective is reported by the rank that had it
 * AFTER the collective's last barrier (its peers complete the step).                                                              */
int hxv_comm_local_create(int32_t nranks, void **group);
int hxv_comm_init_local(hxv_handle *h, void *group);
int hxv_comm_local_abort(void *group);
int hxv_comm_local_destroy(void *group);
/* d_hv_local = (H v)|slab from this rank's slab d_v_local (hxv_localvec_elems() elements each, padded device layout):
 * exchange + product, asynchronous on `stream`.  nranks==1 without a communicator: the plain product.              */
int hxv_apply_device_slab(hxv_handle *h, const void *d_v_local, void *d_hv_local, void *stream);
/* Measurement: nrep such products on the handle's own stream, timed with HIP events (collective on a split sector: every rank calls
 * it with the same nrep).  *ms_step = mean time of a whole product on this rank (exchange included), *ms_kernels = mean time of its
 * product kernels alone (both kernel regions in exchange mode 2; with option "exchange_overlap" also pass A's region on the second stream,
 * which runs BESIDE the exchange: hxv_get_option(h, "time_kernels_overlapped_us") tells that part, so the exchange's own share of a step is
 * *ms_step - (*ms_kernels - overlapped), never negative).                                                                        */
int hxv_time_apply_slab(hxv_handle *h, const void *d_v_local, void *d_hv_local, int32_t nrep, float *ms_step, float *ms_kernels);
/* Where the exchange wants this rank's slab (its slot of the gather buffer): a caller that builds its vector there and hands
 * THAT pointer to hxv_apply_device_slab saves the slab copy of every product.  [qdw columns][pitch] complex elements; allocated on
 * first use; valid until hxv_comm_free / hxv_destroy; the device Lanczos drivers of a split sector keep their own vectors at the same
 * place, so a vector left there does not survive a driver call -- a START vector of hxv_lanczos_tridiag[_pair] built there is fine: the
 * drivers stage it (one slab copy per run) before they clear the place.  The reference allocates the gathered vector per call and
 * copies (ED_HAMILTONIAN_SPARSE_HxV.f90:277-296).                                                                              */
int hxv_slab_home(hxv_handle *h, void **d_slab);
/* Exchange mode 2 (hxv_set_exchange_default(2) / HXV_EXCHANGE=alltoall before the sector is opened; not with the spH0nd block): the
 * reference's own two transposes (vector_transpose_MPI, ED_HAMILTONIAN_COMMON.f90:30-94; spMatVec_mpi_main :272-296) inside the
 * engine -- slab -> row panels (rows split like the columns, :274-275), dw hops on the panel, back, then diagonal + up hops on the slab.
 * Moves (P-1)/P of one slab per rank and transpose instead of P-1 slabs: the lowest-traffic exchange.  hxv_apply_host,
 * hxv_apply_device_slab and the device drivers (REAL-vector mode included) use it transparently; hxv_slab_home does not apply.   */
int64_t hxv_exchange_count(const hxv_handle *h); /* exchanges since creation */
/* HALO exchange (the lower-traffic alternative, replaces the transposes of ED_HAMILTONIAN_COMMON.f90:30-94 differently): with
 * the reference's own DimDw split a rank's rows of H_dw reference only a subset of the other ranks' columns (C3, 8 ranks:
 * 4.2 slabs instead of the 7 an all-gather moves).  A handle created in halo mode (hxv_set_exchange_default(1) or
 * HXV_EXCHANGE=halo before the create call; with Jx / Jp the partner columns of the spH0nd block's dw moves join the list) expects d_v_full of hxv_apply_device in the HALO
 * LAYOUT: its own qdw columns first, then the columns listed by hxv_halo_lists (ascending = grouped by owner rank);
 * hxv_fullvec_elems() reports the length.  hxv_apply_host / hxv_apply_device_slab / the drivers then exchange exactly
 * those columns (grouped ncclSend/ncclRecv).  recv_counts/send_counts: columns per peer rank; recv_cols: global column
 * indices in slot order; send_cols: LOCAL column indices grouped by destination rank.                                */
int hxv_set_exchange_default(int32_t mode); /* 0 all-gather [default], 1 halo, 2 two all-to-all transposes; applies to handles created afterwards */
int32_t hxv_exchange_mode(const hxv_handle *h);
int hxv_halo_counts(const hxv_handle *h, int32_t *recv_counts, int32_t *send_counts);
int hxv_halo_lists(const hxv_handle *h, int32_t *recv_cols, int32_t *send_cols);
/* The halo PLAN of any rank of any split, computed from H_dw alone (CSR as hxv_get_csr returns it / as spH0dws(1) stores it:
 * 1-based columns) -- no handle, no device, no communicator: counts[nranks] columns per peer; recv_cols (slot order) and send_cols
 * (grouped by destination) as GLOBAL 0-based column indices, *n_recv / *n_send their lengths (call once with NULL lists to size
 * them).  What one process needs to check that rank p's send list towards q IS rank q's receive list from p, for every pair.
 * (The hopping part only: a sector with Jx / Jp adds the spH0nd partners -- hxv_halo_lists of its handle is the full list.)      */
int hxv_halo_plan_from_csr(int32_t dimdw, const int64_t *dw_rowptr, const int32_t *dw_cols, int32_t rank, int32_t nranks,
                           int32_t *recv_counts, int32_t *send_counts, int32_t *recv_cols, int32_t *send_cols, int32_t *n_recv,
                           int32_t *n_send);

/* Device-resident product.  d_v_full: the FULL vector in the ALL-GATHER LAYOUT: nranks slabs of
 * cmax*pitch elements each, cmax = ceil(DimDw/nranks), slab r holding rank r's columns (ranks
 * that own one column less leave their last pitch elements unused) -- exactly what an
 * equal-count ncclAllGather / MPI_Allgather of the padded slabs produces; hxv_fullvec_elems()
 * elements in all.  d_hv_local: this rank's slab (hxv_localvec_elems() elements), overwritten.  Asynchronous on `stream` (a hipStream_t; NULL = the legacy
 * default stream, as in every HIP API), so it orders with the caller's other work on that
 * stream.  d_v_full and d_hv_local must not overlap.
 * When H is real (hxv_real_vectors_available) one complex product is two independent real products, H(x + i y) =
 * Hx + i Hy: a caller with several real vectors to multiply (the Green's-function channels of one solve) gets two
 * per call at 4.4 ms (C3) instead of 2.9 ms each through hxv_apply_device_real.                                     */
int hxv_apply_device(hxv_handle *h, const void *d_v_full, void *d_hv_local, void *stream);
/* DEVICE VECTOR LAYOUT.  On the device every column of DimUp elements is padded to hxv_pitch(h) =
 * DimUp rounded up to a multiple of 8 elements, so each column starts on a 128-byte line; element
 * (iup, column slot k) lives at k*pitch + iup.  The pad rows are never read as sources and never written by
 * the product; the Lanczos entries require them to be ZERO in the vectors they are given (dot products
 * run over the padded arrays).  hxv_apply_host converts from/to the reference's contiguous host layout.
 *   hxv_fullvec_elems : length of d_v_full  = nranks*cmax*pitch  (all-gather layout above)
 *   hxv_localvec_elems: length of d_hv_local and of every Lanczos vector = qdw*pitch
 * DEVICE ROW ORDER (round 6).  WITHIN a column the rows of a device vector need not follow the reference's basis order: a sector opened from a
 * model may store the up configurations in the order they take when the orbitals are renumbered (orbital o at bit pos[o]) so that the
 * out-of-block gathers of the product's up-hop pass run over long contiguous stretches (C3: a third fewer cache lines).
 * Reordering creation operators changes the sign of a basis vector, hence
 *        d_vec[k*pitch + perm[iup]] = sign[iup] * v_ref[k*DimUp + iup]              (perm, sign: hxv_row_order)
 * Every entry point that takes or returns HOST arrays (hxv_apply_host, the *_host drivers, hxv_vector_from_host / _to_host, evecs_host) and
 * every introspection call (hxv_get_maps / _csr / _diag) speaks the reference's order: the conversion happens at the boundary, on the device.
 * Device vectors are self-consistent among the device entry points (product, Lanczos drivers, ladder operators between sectors); a caller
 * that BUILDS or READS a device vector element by element uses hxv_row_order.  Columns (the dw index, the one that is split over ranks)
 * always keep the reference's order.  hxv_row_order returns 1 when the sector has a device row order (perm[DimUp]: reference row -> device
 * row; sign[DimUp]: +1 / -1 by reference row; either may be NULL), 0 when rows are in the reference's order (identity written), -1 on a NULL
 * handle.  Sectors opened from stored matrices, row panels and small sectors (DimUp < 2048) keep the reference's order; environment
 * HXV_ROW_ORDER=0 keeps it everywhere.                                                                                                 */
int32_t hxv_row_order(const hxv_handle *h, int32_t *perm, int8_t *sign);
int64_t hxv_fullvec_elems(const hxv_handle *h);
int64_t hxv_localvec_elems(const hxv_handle *h);
int32_t hxv_pitch(const hxv_handle *h);

/* ---- the two halves of the product, for the reference's own all-to-all exchange (ED_HAMILTONIAN_SPARSE_HxV.f90:272-296)
 * instead of the all-gather: rank r first receives the row panel X = v[rows U_r, ALL columns] (rows split like the
 * columns, mpiQup :274-275), computes Y = X H_dw^T with a PANEL handle, sends Y's column ranges back to their owners, and
 * finishes with  hv = D.v + H_up v + (assembled dw part)  on its own slab.  Each transpose moves (P-1)/P of a slab
 * instead of (P-1) slabs.
 * hxv_create_dw_panel : handle for a panel of `nrows` rows (dw-only: no basis/H_up/diagonal for the up index);
 *                       vectors are [DimDw columns][pitch = roundup8(nrows)].
 * hxv_apply_dw_panel  : d_y = d_x H_dw^T, same layout in and out.
 * hxv_apply_up_add    : d_hv_local = D.v + H_up v + d_w on the local slab; d_v_local and d_w are [qdw columns][pitch]
 *                       (d_v_local = this rank's slab only -- no gathered vector); not available with spH0nd (Jx/Jp).
 * Like the product, both halves never read the pad rows of their inputs and never write the pad rows of their outputs. */
int hxv_create_dw_panel(const hxv_model *model, int32_t nup, int32_t ndw, int32_t nrows, int32_t device, hxv_handle **out);
int hxv_apply_dw_panel(hxv_handle *panel, const void *d_x, void *d_y, void *stream);
int hxv_apply_up_add(hxv_handle *h, const void *d_v_local, const void *d_w, void *d_hv_local, void *stream);

/* ---- REAL-vector mode.  When every amplitude of H is real (cdn_hm_* models; not BHZ), H maps real vectors to real
 * vectors, and a Lanczos run started from a real vector never leaves the reals: the same kernels then run on
 * double instead of complex(8) elements -- half the bytes of every pass.  The reference keeps complex arrays
 * throughout (cc_sparse_HxV, ED_VARS_GLOBAL.f90:72-78), so this mode exists only on the device side: the device
 * Lanczos drivers below select it by themselves when it applies (option "real_vectors", default 1) and convert at
 * their boundaries; hxv_apply_device_real is the product itself.
 *   layout: double[DimDw columns][hxv_pitch_real(h) = roundup16(DimUp)], pad rows zero / ignored like above.
 *   available iff H is real, the tiled kernels are in use, no spH0nd block (hxv_real_vectors_available).  On a split sector
 *   the drivers exchange REAL slabs (half the bytes on the links); hxv_apply_device_real itself takes the whole vector of an
 *   unsplit sector.                                                                                                  */
int32_t hxv_real_vectors_available(const hxv_handle *h);
int32_t hxv_pitch_real(const hxv_handle *h);
int64_t hxv_realvec_elems(const hxv_handle *h);
int hxv_apply_device_real(hxv_handle *h, const void *d_v_real, void *d_hv_real, void *stream);

/* Time `nrep` back-to-back device products with HIP events recorded on the stream the
 * kernels are launched on; returns the mean milliseconds per product.                    */
int hxv_time_apply(hxv_handle *h, const void *d_v_full, void *d_hv_local, int32_t nrep, float *ms_per_apply);

/* ---- Lanczos on device (SciFortran sp_lanc_tridiag / sp_lanc_eigh call shapes,
 * ED_GF_NORMAL.f90:215-220, ED_DIAG.f90:176-184).  Split sectors (nranks>1) after hxv_comm_init:
 * vectors are this rank's slab, dot products are all-reduced; the fused recurrence and the REAL-vector mode apply there too
 * (the epilogue's partial sums are a rank's share of alpha).  A rank that fails in its local preparations tells the others before
 * the first collective: all ranks return an error together instead of waiting for each other.
 * All vectors in the padded device layout (hxv_localvec_elems() elements, pad rows zero).
 * tridiag: d_vin = start vector (normalised by the driver if it is not, as SciFortran does); alanc[nlanc], blanc[nlanc]
 *   filled as alanc(k)=<q_k|H|q_k>, blanc(k+1)=beta_{k+1}, blanc(1)=0 (ED_GF_NORMAL.f90:949-951);
 *   *nsteps = iterations done (early exit when beta < threshold).
 * eigh: lowest eigenvalue *egs and eigenvector d_vect (device, Dim, written) from a
 *   deterministic start vector; stops when |dE| < threshold (and, if d_vect is wanted, the Ritz
 *   residual estimate |beta*y_last| < 1e-11*max(1,|E|)) or at nitermax (ED_DIAG.f90:176).
 * tridiag with nlanc >= 8 runs iterations 1.. on the device alone (scalars in device memory, three iterations per
 *   hipGraph, alanc/blanc copied back once; option "lanczos_graph", default 1): bit-identical to the stepwise run.
 * REAL-vector mode (above): with option "real_vectors" = 1 (default) these drivers and hxv_eigh_lowest run on real
 *   vectors whenever hxv_real_vectors_available(h) and the start vector is real (eigh / eigh_lowest: the engine's own
 *   start vector is then real; tridiag: d_vin must have exactly zero imaginary part, else the complex path runs).
 *   Inputs and outputs keep the complex layout; alanc/blanc/E are the same numbers.  hxv_get_option(h,"lanczos_real_last")
 *   tells which path the last run took.                                                               */
int hxv_lanczos_tridiag(hxv_handle *h, const void *d_vin, int32_t nlanc, double *alanc, double *blanc, double threshold,
                        int32_t *nsteps);
int hxv_lanczos_eigh(hxv_handle *h, int32_t nitermax, double threshold, double *egs, void *d_vect, int32_t *niter);
/* Same two drivers with HOST vectors in the reference's contiguous layout (what ED_DIAG / ED_GF_NORMAL hold):
 * one PCIe copy per Lanczos RUN instead of two per iteration.  vin_host: Dim complex, normalised by the caller;
 * vect_host: Dim complex, written (may be NULL).  These are what the Fortran glue's gpu_sp_lanc_tridiag /
 * gpu_sp_lanc_eigh (SciFortran call signatures) forward to.                                                 */
int hxv_lanczos_tridiag_host(hxv_handle *h, const void *vin_host, int32_t nlanc, double *alanc, double *blanc, double threshold,
                             int32_t *nsteps);
int hxv_lanczos_eigh_host(hxv_handle *h, int32_t nitermax, double threshold, double *egs, void *vect_host, int32_t *niter);
/* TWO tridiagonalisations on one product, for real H (hxv_real_vectors_available): the Green's-function channels of one solve
 * are independent runs of sp_lanc_tridiag (ED_GF_NORMAL.f90:123-306, one per call site :215,282,422,504,638,720,801,882), and
 * a complex product IS two real ones, H(x + i y) = H x + i H y.  The two REAL start vectors (complex layout, imaginary parts
 * exactly zero -- c / c^dagger applied to a real ground state; refused otherwise) travel as real and imaginary part of one
 * complex Lanczos vector; every scalar of the recurrence, every dot product and both early exits exist once per component.
 * alanc_x/blanc_x[nlanc], *nsteps_x as in hxv_lanczos_tridiag.  Each component's numbers are bit-identical to
 * hxv_lanczos_tridiag on that start vector through the same kernels, i.e. with option real_vectors = 0 (the complex-vector path; any job_up).
 * Against hxv_lanczos_tridiag's DEFAULT path (real_vectors = 1: the real-vector kernels, another summation order) they agree to rounding, not bit
 * for bit -- 1e-10 over the first steps, growing with the step like any two Lanczos runs; the continued fraction the consumer builds from them
 * (ED_GF_NORMAL.f90:915-975) agrees to 1e-9 (tests/test_gpu_lanczos.py::test_paired_tridiagonalisation_..., tests/test_gpu_solve_sweep.py).
 * Split sectors: slabs per rank, every sum all-reduced (any exchange).  The _host form takes the start vectors in the reference's
 * contiguous host layout.
 * What does NOT pair: the (c^+_i + xi c^+_j)|gs>, (c_i - xi c_j)|gs> channels of the reference's default chan4 form (ED_GF_NORMAL.f90:746-780,
 * :827-861) have COMPLEX start vectors even at real H -- 24 of the 56 runs of a 2x2 solve; they go through hxv_lanczos_tridiag on complex
 * vectors (C3: 5.5 ms per step against 2.8 ms per paired real channel-step).  For real symmetric H they carry nothing the real channels do
 * not; the reference's own ed_gf_symmetric (chan2) drops them: INTEGRATION.md section 4.                                            */
int hxv_lanczos_tridiag_pair(hxv_handle *h, const void *d_vin_a, const void *d_vin_b, int32_t nlanc, double *alanc_a, double *blanc_a,
                             double *alanc_b, double *blanc_b, double threshold, int32_t *nsteps_a, int32_t *nsteps_b);
int hxv_lanczos_tridiag_pair_host(hxv_handle *h, const void *vin_a_host, const void *vin_b_host, int32_t nlanc, double *alanc_a,
                                  double *blanc_a, double *alanc_b, double *blanc_b, double threshold, int32_t *nsteps_a,
                                  int32_t *nsteps_b);
/* ---- OFF-DIAGONAL Green's functions from one run per orbital.  The reference recovers G_ij from three diagonal-type continued fractions,
 * G_ij = 1/2 (G_{i+j} - G_ii - G_jj), and runs a tridiagonalisation per mixed start vector for it (lanc_build_gf_normal_mix_chan2/4,
 * ED_GF_NORMAL.f90:315-903: 48 of the 56 runs of a 2x2 solve).  The Krylov space of v = c^dagger_i|gs> already holds the Galerkin solution of
 * (z - H) x = v,  x_m(z) = |v| sum_k q_k [(z - T)^{-1}]_{k1},  so <p|(z - H)^{-1}|v> for any other vector p needs only the overlaps
 * o_k = <p|q_k> of the Lanczos vectors with p, collected while the run for G_ii is under way: one extra streaming pass per step over the
 * Lanczos vector and the probes.  H Q = Q T + beta q_{m+1} e_m^T holds locally to rounding whether or not the q_k stay orthogonal, so the
 * result does not rely on re-orthogonalisation.
 * hxv_lanczos_tridiag_probes: hxv_lanczos_tridiag with up to HXV_MAX_PROBES probe vectors.
 *   alanc, blanc, *nsteps : what hxv_lanczos_tridiag returns for the same d_vin on the same handle, bit for bit, whenever both take the same
 *     vector path (below): the same recurrence, run through the host-stepped loop (the graph-captured path is bit-identical to it; a split
 *     sector runs the host loop anyway).  The start vector is normalised by the driver when it is not.
 *   overlaps[2*(k*nprobes + j)], [.. + 1] = Re, Im <p_j|q_k> = sum conj(p_j[i]) q_k[i] for k < *nsteps, q_k the UNIT Lanczos vector of step k
 *     (q_0 = d_vin / |d_vin|); entries of steps that did not run are zero.  The probes are used as given: their norm is the caller's business.
 *     A probe may be d_vin itself: its first overlap is the start vector's norm, the later ones measure the loss of orthogonality.
 *   d_probes : nprobes device vectors of the sector (this rank's slab, hxv_localvec_elems() elements, pad rows zero, like d_vin); nprobes = 0
 *     (d_probes, overlaps may be NULL) is a plain stepwise tridiagonalisation.
 * The overlaps of q_k are computed before the product of step k, in one pass that reads q_k and every probe once (no floating-point atomics:
 * the same vectors give the same bits on every call), and reach the host -- a page-locked staging array of the handle -- with the
 * synchronisation the step makes for alpha and beta.
 * REAL-vector mode: the run is real when hxv_lanczos_tridiag's rule holds (option "real_vectors", H real, Im(d_vin) == 0 on all ranks) AND
 * every probe has zero imaginary part on all ranks -- one reduction for all of them; the probes are then converted once into buffers from the
 * device-buffer cache, which go back before the call returns, and the imaginary parts of the overlaps are exactly zero.  Otherwise the
 * complex path runs (a complex probe of a real start vector: alanc / blanc then equal hxv_lanczos_tridiag's with option "real_vectors" = 0).
 * "lanczos_real_last" reports the path.  No basis maps are needed: handles from hxv_create_from_csr, with the spH0nd block, and with option
 * "lanczos_fused" = 0 work alike.
 * SPLIT SECTORS: the rules of hxv_lanczos_tridiag; the 2*nprobes partial sums of a step are summed over the ranks in ONE all-reduce (get
 * "allreduce_count" counts a handle's sum all-reduces); argument and allocation failures are agreed on by all ranks before the first collective
 * step.  A start vector at hxv_slab_home is staged as in hxv_lanczos_tridiag; a PROBE inside one of the handle's gather buffers is refused
 * on every rank together, with nobody left in a collective (HXV_ERR_ARG on the rank whose probe it is; its peers get the error the agreement
 * hands them, HXV_ERR_ARG or HXV_ERR_STATE depending on the transport): the driver clears that place.
 * Errors: HXV_ERR_ARG for a NULL handle, d_vin, alanc, blanc or nsteps, nlanc < 1, nprobes outside [0, HXV_MAX_PROBES], nprobes > 0 with a
 * NULL list, a NULL entry or NULL overlaps, a zero or non-finite start vector.
 * Two probe runs on one product: hxv_lanczos_tridiag_pair_probes below.  Not provided: a graph-captured form, a host-vector form.       */
#define HXV_MAX_PROBES 8
int hxv_lanczos_tridiag_probes(hxv_handle *h, const void *d_vin, int32_t nprobes, const void *const *d_probes, int32_t nlanc, double *alanc,
                               double *blanc, double *overlaps /* [nlanc][nprobes] complex, interleaved, step-major */, double threshold,
                               int32_t *nsteps);
/* TWO probe runs on one product, for real H: hxv_lanczos_tridiag_pair with the overlaps of hxv_lanczos_tridiag_probes for each component.  The
 * runs of a Green's-function solve that share a probe list -- orbitals i, i' of one spin and sector with all c^dagger_j|gs> as probes, or two
 * columns of a susceptibility with all dO_a|psi> -- pay for one product per step between them, and the probes are read once for both.
 *   d_vin_a, d_vin_b, alanc_x, blanc_x, *nsteps_x, threshold : as in hxv_lanczos_tridiag_pair (the same driver: that entry is the nprobes = 0
 *     form of this one, with the same bits); each component has its own scalars and breaks down on its own, the other one then goes on alone.
 *   d_probes : nprobes vectors, 0 .. HXV_MAX_PROBES, in the complex layout like d_vin, shared by both components.  Their imaginary parts must be
 *     exactly zero on all ranks, like the start vectors': ONE reduction checks all of them, every rank sees its sum, and all ranks return
 *     HXV_ERR_ARG together when it is not zero (a complex probe goes through hxv_lanczos_tridiag_probes' complex path).  The probes' real parts
 *     are written once into double buffers on the slab's own index, taken from the device-buffer cache and returned before the call returns.
 *   overlaps_x[2*(k*nprobes + j)] = <p_j|q_k^x> for the UNIT Lanczos vector of component x and step k < *nsteps_x, [.. + 1] = 0 exactly: the
 *     layout of hxv_lanczos_tridiag_probes' overlaps, so hxv_gf_from_probes takes each array as it is.  Entries of steps a component did not
 *     run are zero.
 * Per step one pass over the stored complex vector and the probes, before the product: 16 + 8*nprobes bytes per state for both components (two
 * single real runs read 2*(8 + 8*nprobes)); no floating-point atomics.  Each component's alanc, blanc, nsteps and overlaps are bit-identical
 * to hxv_lanczos_tridiag_probes on that start vector with the same probes through the complex-vector kernels (option real_vectors = 0, any
 * job_up, lanczos_graph = 0); against its default real-vector path they agree to rounding, as for hxv_lanczos_tridiag_pair.
 * "lanczos_real_last" reports 2.  Needs the fused recurrence (option "lanczos_fused" = 1).
 * SPLIT SECTORS: as hxv_lanczos_tridiag_probes -- the 2*nprobes sums of a step in ONE all-reduce, start vectors at hxv_slab_home staged, a probe
 * inside a gather buffer refused on all ranks together.
 * Errors: HXV_ERR_UNSUPPORTED for a complex H or without the fused recurrence; HXV_ERR_ARG for a NULL handle, start vector, alanc or blanc,
 * nlanc < 1, nprobes outside [0, HXV_MAX_PROBES], nprobes > 0 with a NULL list, a NULL entry or a NULL overlaps array, an imaginary part in a
 * start vector or a probe, a zero or non-finite start vector.  Not provided: a graph-captured form, a host-vector form.                  */
int hxv_lanczos_tridiag_pair_probes(hxv_handle *h, const void *d_vin_a, const void *d_vin_b, int32_t nprobes, const void *const *d_probes,
                                    int32_t nlanc, double *alanc_a, double *blanc_a,
                                    double *overlaps_a /* [nlanc][nprobes] complex, interleaved, step-major */, double *alanc_b,
                                    double *blanc_b, double *overlaps_b, double threshold, int32_t *nsteps_a, int32_t *nsteps_b);
/* From the overlaps to poles and weights (pure host code, no device):  T = Z diag(lambda) Z^T  of the nsteps x nsteps tridiagonal matrix
 * (alanc, blanc as returned above; the engine's own implicit QL, no LAPACK),
 *     poles[n] = lambda_n (ascending),   weights[2*(n*nprobes + j)], [.. + 1] = Re, Im of  norm * Z_{1n} * sum_k o_kj Z_kn,
 * so that  <p_j|(z - H)^{-1}|v>  ~  sum_n weights[n][j] / (z - poles[n]),  norm = |v| of the UNNORMALISED start vector (the square root of
 * hxv_apply_ladder's *norm2).  For p = v (the unnormalised d_vin given as a probe of its own run) the weight is norm^2 Z_{1n}^2, the reference's own formula
 * (ED_GF_NORMAL.f90:949-973).  In the reference's conventions (add_to_lanczos_gf_normal, :915-975) the channel c^dagger (isign = +1) adds
 * weights / (z - (poles - E0)) and the channel c (isign = -1) adds weights / (z + (poles - E0)) to impGmatrix, E0 the ground-state energy.
 * With v = c^dagger_i|gs> and p_j = c^dagger_j|gs> the sum is the particle part of G_ji; with v = c_i|gs>, p_j = c_j|gs> and the pole sign
 * flipped it is the hole part of G_ij.
 * Errors: HXV_ERR_ARG for nsteps < 1, nprobes < 0 or a NULL array (overlaps / weights may be NULL when nprobes == 0); HXV_ERR_STATE when the
 * QL iteration does not converge.                                                                                                      */
int hxv_gf_from_probes(int32_t nsteps, const double *alanc, const double *blanc, int32_t nprobes, const double *overlaps,
                       double norm /* |v| of the unnormalised start vector */, double *poles /* [nsteps] */,
                       double *weights /* [nsteps][nprobes] complex */);
/* ---- CHEBYSHEV RECURRENCE: functions of H applied to a device-resident state, and spectral moments with a uniform resolution.  With the
 * window  Ht = (H - b)/a,  spectrum of H inside [b - a, b + a]  (hxv.chebyshev.spectral_window gives one), the vectors
 *     t_0 = v,   t_1 = Ht v,   t_{n+1} = 2 Ht t_n - t_{n-1}      (t_n = T_n(Ht) v)
 * carry every polynomial of H: e^{-tau H} v (thermal typical states), e^{-iHt} v (real-time propagation), spectral filters, and the moments
 * of the kernel polynomial method.  Per order: ONE product (the engine's own, through the slab product without an epilogue) and ONE fused
 * streaming pass that forms t_{n+1} over t_{n-1}, adds c_{n+1} t_{n+1} to the running sum, and reduces the overlaps with the probes together
 * with <t_{n+1}|t_{n+1}> and <t_{n+1}|t_n>; (3 + M)*16 bytes per state for M probes, (4 + M)*16 with a running sum.  No floating-point
 * atomics: the same vectors on the same handle give the same bits on every call.  These two entries run on COMPLEX vectors whatever H is,
 * and option "real_vectors" does not apply to them; for a real H with real vectors the REAL-vector forms below do the same work at half
 * the bytes.  The choice is the caller's, by the entry's name: nothing selects the real path automatically.
 * hxv_chebyshev_moments:
 *   moments[2*(n*nprobes + j)], [.. + 1] = Re, Im <p_j|T_n(Ht)|v> = sum conj(p_j[i]) t_n[i]  for n < nmom, from nmom - 1 products.  d_probes as
 *     in hxv_lanczos_tridiag_probes (used as given; a probe may be d_vin itself); nprobes = 0: d_probes and moments may be NULL.
 *   self_moments[k] = <v|T_k(Ht)|v> for k <= 2*nmom - 2, from the same products:  mu_0 = <v|v>,  mu_1 = Re<t_1|t_0>,
 *     mu_{2n} = 2<t_n|t_n> - mu_0,  mu_{2n+1} = 2 Re<t_{n+1}|t_n> - mu_1.  May be NULL.
 *   d_vin is used as given, NOT normalised, and only read.
 * hxv_chebyshev_apply:
 *   d_out = sum_{n < ncoef} coef_n T_n(Ht) v,  coef[2n], [2n+1] = Re, Im coef_n (hxv.chebyshev.exp_coefficients / propagator_coefficients);
 *   *norm2 = <d_out|d_out> (may be NULL).  d_vin is only read; d_out == d_vin is refused.  ncoef - 1 products.
 * SCRATCH: three vector-sized blocks and one small one from the device-buffer cache, back there on every way out ("pool_live_blocks").
 * WINDOW GUARD: for a spectrum inside the window |t_n| <= |v|.  After EVERY order the driver compares <t_n|t_n> with 4 <v|v> and returns
 * HXV_ERR_ARG ("spectrum outside the window") when it is larger or when any sum of the order is not finite; 4 is a guard, not a tolerance -- a
 * window that is too narrow grows geometrically and passes it within a few orders.  The sums are read with ONE stream synchronisation per
 * order, on split and unsplit sectors alike (it also delivers the moments): the host's launch latency of the next product, a few tens of
 * microseconds, is exposed once per order.  After such an error d_out holds the partial sum of the orders before it.
 * No basis maps are needed: handles from hxv_create_from_csr, with the spH0nd block, with either job_up work alike.
 * SPLIT SECTORS: this rank's slab, collective; all 2*nprobes + 3 sums of an order in ONE all-reduce, so every rank sees the same sums and
 * all ranks leave together on the guard; argument and allocation failures are agreed on by all ranks before the first collective step.  d_vin
 * is copied before the first exchange, so a start vector at hxv_slab_home is staged (the exchange then overwrites that place); a PROBE or
 * d_out inside one of the handle's gather buffers is refused on every rank together, as in hxv_lanczos_tridiag_probes.  The vectors of the
 * recurrence live in cache blocks, not in the gather buffers: one slab copy per product.
 * Errors: HXV_ERR_ARG for a NULL handle, d_vin, d_out or coef, nmom < 1, ncoef < 1, a <= 0, a non-finite a, b or coefficient, nprobes outside
 * [0, HXV_MAX_PROBES], nprobes > 0 with a NULL list, a NULL entry or NULL moments, a zero or non-finite start vector, a probe whose overlap with the start vector is not finite, and from the
 * guard. */
int hxv_chebyshev_moments(hxv_handle *h, const void *d_vin, int32_t nprobes, const void *const *d_probes, int32_t nmom, double a, double b,
                          double *moments /* [nmom][nprobes] complex, order-major; NULL iff nprobes == 0 */,
                          double *self_moments /* [2*nmom-1] real, may be NULL */);
int hxv_chebyshev_apply(hxv_handle *h, const void *d_vin, int32_t ncoef, const double *coef /* [ncoef] complex */, double a, double b,
                        void *d_out, double *norm2 /* <out|out>, may be NULL */);
/* REAL-VECTOR FORMS of the two entries above, for a real H (every cdn_hm_* model) and purely real d_vin and probes: thermal typical states
 * e^{-beta H/2}|r> and the moments of a real start vector never leave the reals.  The vectors AT THE BOUNDARY stay in the handle's ordinary
 * complex padded layout, as with the Lanczos drivers; inside, the recurrence runs on real blocks double[qdw][pitch_real] from the buffer
 * cache: d_vin and the probes are converted once at the start, d_out is converted back once at the end.  Per order: the real product
 * (apply_slab_real, no epilogue), one real streaming pass -- (3 + M)*8 bytes per state, (4 + M)*8 with a running sum -- ONE all-reduce of
 * nprobes + 2 sums and ONE stream synchronisation.  Windows, guard, self-moment formulas, split sectors (the exchange moves real slabs),
 * refusals of vectors in a gather buffer and the agreement before the first collective are those of the complex entries.
 *   moments[n*nprobes + j] = <p_j|T_n(Ht)|v>, REAL;  self_moments as above;  coef[n] REAL.
 *   d_out: the imaginary part of every element is exactly +0.0.  d_out is written ONLY ON SUCCESS: after any error return it holds what it
 *     held before the call (the running sum lives in a cache block until the last order is done).
 *   SCRATCH: 3 + nprobes (+ 1 with d_out) real vector-sized blocks and one small one, back in the cache on every way out.
 * Option "real_vectors" does NOT gate these entries: the caller asked for the real form by name.
 * Errors: HXV_ERR_UNSUPPORTED, with the blocker's text, where hxv_real_vectors_available(h) is 0 (complex amplitudes, the spH0nd block, the
 * tiled kernels not in use, debug options); HXV_ERR_ARG when d_vin or any probe has a non-zero (or non-finite) imaginary part -- the sum of
 * |Im| over all of them and all ranks in one reduction, so every rank of a split sector decides alike -- and for everything the complex
 * entries refuse. */
int hxv_chebyshev_moments_real(hxv_handle *h, const void *d_vin, int32_t nprobes, const void *const *d_probes, int32_t nmom, double a,
                               double b, double *moments /* [nmom][nprobes] REAL, order-major; NULL iff nprobes == 0 */,
                               double *self_moments /* [2*nmom-1] real, may be NULL */);
int hxv_chebyshev_apply_real(hxv_handle *h, const void *d_vin, int32_t ncoef, const double *coef /* [ncoef] REAL */, double a, double b,
                             void *d_out, double *norm2 /* <out|out>, may be NULL */);
/* A SEEDED RANDOM STATE on the device: the start vector of the typical-state methods, without numpy over Dim elements and a host-to-device
 * copy.  Local, not collective; any handle (hxv_create_from_csr included), no basis maps needed.  ONE streaming kernel writes every element
 * of d_vec (hxv_localvec_elems() elements, padded layout), pad rows zero, and the call returns when it is done.
 * The value of an element depends only on (seed, I, c), I = col * DimUp + reference row the GLOBAL index in the reference's order, c the
 * component, so a sector gets the same vector whatever its device row order, rank split or handle kind (hxv_vector_to_host gives the same
 * host array).  With mix(x) the splitmix64 finaliser  x += 0x9E3779B97F4A7C15;  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 * x = (x ^ (x >> 27)) * 0x94D049BB133111EB;  x ^ (x >> 31)  (64-bit wrap-around arithmetic):
 *     key = mix(seed),     u(I, c) = (double)(mix(key ^ (2*I + c)) >> 11) * 2^-53 - 0.5          uniform in [-0.5, 0.5)
 *     complex_valued = 0:  element I = (u(I, 0), +0.0 exactly);      complex_valued = 1:  element I = (u(I, 0), u(I, 1)).
 * Vectors of different seeds are independent samples (the key is hashed before it meets the index: no seed is a shifted copy of another);
 * not normalised: <v|v> ~ Dim/12 per component.
 * Errors: HXV_ERR_ARG for a NULL handle or vector, complex_valued outside {0, 1}. */
int hxv_vector_random(hxv_handle *h, uint64_t seed, int32_t complex_valued, void *d_vec);
/* ---- Several lowest eigenpairs on device: the call SciFortran's sp_eigh (P-ARPACK) serves at ED_DIAG.f90:152-160,
 *   call sp_eigh(spHtimesV_p, eig_values(Neigen), eig_basis(vecDim,Neigen), Nblock, Nitermax, tol=lanc_tolerance)
 * as a thick-restart Lanczos (the explicit-restart form of ARPACK's implicitly restarted Lanczos for Hermitian
 * operators) with a Krylov basis of ncv (= Nblock) vectors resident in HBM, full re-orthogonalisation and ARPACK's
 * convergence test |beta*s_mi| <= tol*max(eps^(2/3),|theta_i|)  (tol below machine epsilon -- the reference's default
 * lanc_tolerance=1e-18 -- is raised to epsilon).  Serial and split sectors (below).
 *   neigen       : number of lowest eigenpairs wanted (Neigen)
 *   ncv          : basis size (Nblock = lanc_ncv_factor*Neigen+lanc_ncv_add, ED_DIAG.f90:96); <=0 -> 10*neigen; max 64
 *   maxrestart   : restart limit (Nitermax)
 *   evals        : [neigen] ascending
 *   d_evecs      : device, neigen consecutive vectors of hxv_localvec_elems() elements (padded layout), or NULL
 *   evecs_host   : host, eig_basis(Dim,neigen) in the reference's contiguous layout, or NULL
 *   *nconv       : how many of the neigen pairs met the test; *nmatvec: H x V products spent.
 * Needs (ncv+1) vectors of HBM; fails with HXV_ERR_HIP and a message naming the shortfall otherwise.
 * A single Krylov space sees ONE vector of an exactly degenerate level -- ARPACK included: sp_eigh returns further copies only when
 * rounding happens to bring them up, while ED_DIAG.f90:234-244 keeps every state within gs_threshold of the minimum.  DEFAULT = what
 * ARPACK does: one Krylov space, no extra work.  Option "eigh_degenerate" = 1 ASKS for the copies: once the wanted pairs have converged
 * they are locked and the same iteration in their orthogonal complement looks for a state below the current neigen-th lowest value (a
 * hidden copy), repeatedly -- a round that finds nothing stops once the residual bound of its lowest Ritz value clears the level (C3: 380 products + 60; C2: up to as many again); every step of such a round
 * removes the locked eigenvectors (they are converged to `tol` only).  "Nothing below" is a HEURISTIC answer: the lowest Ritz value of
 * the complement minus its residual must clear the level from the second restart cycle on, with a falling residual -- a copy whose
 * overlap with the start vector is at rounding level can still be missed.  *nmatvec counts both; hxv_get_option(h,
 * "eigh_last_search_products" | "eigh_last_check_products") splits it.  Clusters with a non-abelian point group (the 2x2 plaquette: D4)
 * DO have degenerate levels inside a sector: INTEGRATION.md section 3 says when to ask.
 * Split sectors: after hxv_comm_init (vectors = slabs).  If Dim <= ncv the Krylov space closes and all returned pairs are exact. */
int hxv_eigh_lowest(hxv_handle *h, int32_t neigen, int32_t ncv, int32_t maxrestart, double tol, double *evals, void *d_evecs,
                    int32_t *nconv, int32_t *nmatvec);
int hxv_eigh_lowest_host(hxv_handle *h, int32_t neigen, int32_t ncv, int32_t maxrestart, double tol, double *evals,
                         void *evecs_host, int32_t *nconv, int32_t *nmatvec);
/* Time nrep full Lanczos iterations (HxV + recurrence + 2 reductions) on device. */
int hxv_time_lanczos(hxv_handle *h, void *d_work3 /* 3*hxv_localvec_elems() complex */, int32_t nrep, float *ms_per_iter);

/* ---- Green's-function start vectors (ED_GF_NORMAL.f90:174-214: the reference applies c / c^dagger to the
 * ground state serially on the master and scatters): d_out = c^(dagger)_{orbital,spin} d_psi, from the sector
 * open in `from` (vector of its Dim) into the sector open in `to` (N_spin +- 1; vector of its Dim), sign =
 * (-1)^(# occupied orbitals of the SAME spin below `orbital`) (c/cdg, ED_SETUP.f90:807-833; no cross-spin sign,
 * as in the reference).  orbital is 0-based (= pos-1), spin 0 = up, 1 = dw, create 1 = c^dagger, 0 = c.
 * *norm2 = <out|out> (the reference normalises by it, ED_GF_NORMAL.f90:197-199).  Both handles from_model, same device; padded
 * device layouts, d_out's pad rows are written as zero.
 * SPLIT sectors (both handles with the same rank / nranks, `to` with its communicator): d_psi / d_out are this rank's slabs and
 * every rank builds its own slab of the new vector -- the master-only loop + scatter of ED_GF_NORMAL.f90:174-214 is gone.
 * A spin-up operator is local to a slab (both sectors share DimDw and its split); a spin-dw operator maps whole columns of
 * one split onto the other: every rank derives from the two dw maps what it needs from whom and what the others need from it,
 * and one column exchange moves them.  *norm2 is the GLOBAL <out|out>.
 * A spin-dw operator keeps the row, so HXV_ERR_STATE (split or not, d_out untouched) when the two sectors store their rows in
 * different device row orders (HXV_ROW_ORDER or its hooks changed between the opens).                                         */
int hxv_apply_ladder(hxv_handle *from, hxv_handle *to, int32_t orbital, int32_t spin, int32_t create, const void *d_psi,
                     void *d_out, double *norm2);
/* Mixed channels (ED_GF_NORMAL.f90:370-406 (c^dagger_i + c^dagger_j)|gs>, :746-780 (c^dagger_i + xi c^dagger_j)|gs>, and the
 * c_i + c_j / c_i - xi c_j counterparts): d_out = (accumulate ? d_out : 0) + (coef_re + i coef_im) * c^(dagger) d_psi;
 * *norm2 = <out|out> after the update.  With accumulate != 0 the caller's d_out must have zero pad rows.     */
int hxv_apply_ladder_axpy(hxv_handle *from, hxv_handle *to, int32_t orbital, int32_t spin, int32_t create, double coef_re,
                          double coef_im, int32_t accumulate, const void *d_psi, void *d_out, double *norm2);

/* ---- twin-sector eigenstates (ed_twin) --------------------------------------------------------------------------------------
 * With ed_twin the reference solves one sector of every pair A = (nup,ndw), B = (ndw,nup) (ED_SETUP.f90:353-362), stores each eigenstate
 * once with a twin link (ED_DIAG.f90:84,231) and lets every consumer rebuild B's vector through es_return_cvector,
 * vector(i) = twin%cvec(Order(i)) (ED_EIGENSPACE.f90:485-494), Order = twin_sector_order (ED_SETUP.f90:854-898): the argsort of the
 * spin-flipped Fock states, i.e. the transpose of the DimUp x DimDw amplitude matrix,
 *     v_B[idw_A + iup_A*DimDw_A] = v_A[iup_A + idw_A*DimUp_A].
 * hxv_twin_vector does that on the device: d_psi is a device vector of `from` (sector A), d_out one of `to` (sector B = (ndw,nup) of the
 * same Ns), both in the padded device layout; pad rows of d_psi are never read, every element of d_out is written, its pad rows as zero.
 * It runs on `to`'s stream and returns when done.  from == to with nup == ndw is allowed: the spin-flip map on that sector.
 * THE MAP CARRIES NO SIGN, as in the reference.  It is data movement and is defined for any model, but the result is an eigenstate of B
 * only for spin-symmetric models (H_up = H_dw: H_B = T H_A T^t exactly); the reference only warns for Nspin > 1, and so does this comment:
 * nothing is refused on those grounds.
 * DEVICE ROW ORDER: each sector's own order and basis signs apply on its side,
 *     d_out[kB*pitch_B + rB] = sB[rB] * sA[rA] * d_psi[kA*pitch_A + rA],   kB = iperm_A[rA],  kA = iperm_B[rB]
 * (rA, rB device rows; iperm: device row -> reference row, the inverse of hxv_row_order's perm; s: the basis sign of a device row), so the
 * result is what hxv_vector_to_host / transpose / hxv_vector_from_host would give, bit for bit, whether none, one or both sectors have an order.
 * SPLIT SECTORS: two handles that are both rank r of the same nranks > 1.  d_psi is this rank's slab of A, the columns idw in [dw0_A,
 * dw0_A+qdw_A); d_out is this rank's slab of B, B's columns kB in [dw0_B, dw0_B+qdw_B), which are the REFERENCE up-rows of A in that range
 * (DimDw_B = DimUp_A, both split by the one rule of ED_HAMILTONIAN.f90:93-105).  The result is the unsplit map restricted to the slab,
 *     d_out[(kB-dw0_B)*pitch_B + perm_B[idw]] = sB[idw] * sA[kB] * d_psi[(idw-dw0_A)*pitch_A + perm_A[kB]]
 * with each idw taken from the slab of the rank that owns it (perm, s: hxv_row_order's map and sign; the identity and +1 without a row
 * order): bit for bit the same columns as the unsplit call.  The twin of a DimDw split is a DimUp split, so the call is COLLECTIVE over
 * `to`'s communicator (hxv_comm_init or hxv_comm_init_local; `from` need not be bound, as in hxv_apply_ladder): every rank packs its slab
 * by destination, ONE grouped send/receive moves the blocks, every rank unpacks (the reference gathers the whole vector on the master:
 * es_return_cvector_mpi, ED_EIGENSPACE.f90:498-569).  Independent of the product's exchange mode.  Pad rows of d_psi are never read, d_psi
 * is unchanged, every element of d_out is written, pad rows as zero; runs on `to`'s stream and returns when done on this rank; the two
 * staging buffers (about one slab each) come from the device-buffer cache and go back before the call returns.  nranks > min(DimUp_A,
 * DimDw_A) cannot arise: hxv_create_from_model refuses nranks > DimDw for either sector, and a pair opened under the communicator-shrink
 * rule (nranks' = DimDw) has different nranks and is refused below.  hxv_get_option(to, "twin_last_pack_us" / "twin_last_exchange_us" /
 * "twin_last_unpack_us"): what the three phases of the last split call took on the stream (HIP events; -1 before the first).
 * Errors: HXV_ERR_ARG for a NULL argument, handles on different devices, d_out == d_psi, or `to` not the sector (ndw,nup) of `from` with
 * the same Ns; HXV_ERR_STATE for handles without basis maps (from CSR, dw panels), and for two handles split alike whose `to` is not bound
 * to a communicator; HXV_ERR_UNSUPPORTED when the two handles' (rank, nranks) differ (unsplit with split, 2 ranks with 3, rank 0 with
 * rank 1) or an unsplit handle is bound to a communicator.  All of these are decided from the arguments alone, the same on every rank:
 * they return at once, before any collective step, and write nothing.  A rank-local resource failure (staging buffers, table upload) is
 * agreed on by all ranks before the exchange: every rank returns an error, none waits for a peer that has left.  */
int hxv_twin_vector(hxv_handle *from, hxv_handle *to, const void *d_psi, void *d_out);
/* The plan of the split map, not the transport: how many 16-byte elements rank `rank` of an `nranks`-way split sends to and receives from
 * every rank (own entry included: that block stays on the device) when A has dimup_a x dimdw_a amplitudes -- no handle, no device, no
 * communicator, in the spirit of hxv_halo_plan_from_csr; hxv_twin_vector itself sizes and addresses its buffers with these numbers.  The
 * block p -> q holds B's columns of q (qdw_B(q), split of dimup_a) times A's columns of p (qdw_A(p), split of dimdw_a), each block row
 * padded to a multiple of 8 elements: send_counts[q] = qdw_B(q) * roundup8(qdw_A(rank)), recv_counts[p] = qdw_B(rank) * roundup8(qdw_A(p)).
 * HXV_ERR_ARG: a dimension < 1, rank outside [0, nranks), nranks > min(dimup_a, dimdw_a), a NULL array.  */
int hxv_twin_split_plan(int32_t dimup_a, int32_t dimdw_a, int32_t rank, int32_t nranks, int64_t *send_counts, int64_t *recv_counts);

/* ---- impurity observables of device-resident states --------------------------------------------------------------------------
 * ED_OBSERVABLES.f90 lanc_observables (:94-236), lanc_local_energy (:246-452) and the single-particle density matrix of
 * density_matrix_impurity (:609-686), without the eigenvector on the host.  The impurity orbitals are the low Nimp = Nlat*Norb bits of
 * each spin's configuration (is = iorb + ilat*Norb, 0-based; ED_SETUP.f90:563-568), and every quantity of those routines is a function of
 * one RAW RECORD per state, hxv_obs_record_elems() doubles:
 *   [0, 4^Nimp)                         W[a_up + 2^Nimp*a_dw]  weight * |psi|^2 summed over the basis states with impurity bits a_up, a_dw
 *                                                              (= the diagonal of the reference's cluster_density_matrix)
 *   [4^Nimp, 4^Nimp + 2*Nimp^2)          R_up(is,js)  complex, is fastest: weight * sum sgn1*sgn2 * psi_i * conj(psi_j), |j> = c^+_is c_js |i>
 *                                                     (the reference's convention, :644-666); R_up(is,is) = weight * sum n_is |psi_i|^2
 *   [4^Nimp + 2*Nimp^2, + 4*Nimp^2)      R_dw(is,js)  the same for spin dw
 * hxv_observables_accumulate: d_psi is a device vector of h (this rank's slab in the padded layout, device row order included; pad rows are
 * never read).  accumulate == 0 overwrites record, otherwise adds weight * (this state's record) to it; weight is the reference's peso
 * (exp(-beta(Ei-Egs)) / zeta_function, ED_OBSERVABLES.f90:134-135).  Runs on the handle's stream and returns once the record is on the
 * host.  The same vector on the same handle gives the same bits on every call (no floating-point atomics).  Split sectors (after
 * hxv_comm_init / _init_local): collective, every rank returns the GLOBAL record (replaces the Bcast_MPI of :226-233 / :424-430), and all
 * ranks fail together.  Errors: HXV_ERR_ARG for NULL arguments; HXV_ERR_STATE for a handle without basis maps (from CSR, a dw panel);
 * HXV_ERR_UNSUPPORTED for Nimp > 10 (a record over 8 MB).  hxv_obs_record_elems returns 0 for such handles.                          */
int64_t hxv_obs_record_elems(const hxv_handle *h);
int hxv_observables_accumulate(hxv_handle *h, const void *d_psi, double weight, int32_t accumulate, double *record /* host */);
/* The reference's named quantities from a record (pure host code, no device), hxv_obs_derived_elems doubles in this order, each in the
 * reference's Fortran array order:
 *   dens, dens_up, dens_dw, docc, magz (Nlat,Norb);  sz2, n2 (Nlat,Nlat,Norb,Norb);  s2tot (Nlat);
 *   Eknot, Epot (Ehartree included, as :434), Ehartree, Dust, Dund;
 *   single_particle_density_matrix complex (Nlat,Nlat,Nspin,Nspin,Norb,Norb), only ispin == jspin <= Nspin written (:633-666).
 * The fill pattern is the reference's: sz2 / n2 hold (ilat,ilat,iorb,iorb) and, for every jlat, the jorb > iorb pairs and their transposes;
 * Eknot is the real part of its complex sum; the Ust / Jh terms apply for Norb > 1 only.  ONE DELIBERATE DIVERGENCE: Ehartree's constant
 * term uses uloc(iorb) where the reference reads uloc(is) with is = imp_state_index (:399) -- past Norb, and for Nimp > 5 past the 5-element
 * Uloc (ED_INPUT_VARS.f90:19); uloc(iorb) is the intent of the commented line at :395.  Needs Nimp <= 10, Norb <= 5.                    */
int64_t hxv_obs_derived_elems(const hxv_model *model);
int hxv_observables_derive(const hxv_model *model, const double *record, double *out);

/* ---- cluster reduced density matrix of device-resident states ----------------------------------------------------------------
 * ED_OBSERVABLES.f90 density_matrix_impurity (:465-582): rho_imp = Tr_bath |psi><psi|, the reference's cluster_density_matrix (dm_flag),
 * without the eigenvector on the host and without sign factors, as the loop body of :533-568 defines it:
 *   cdm(io,jo) += weight * sum over (b_up,b_dw) of psi(a_up + 2^Nimp b_up, a_dw + 2^Nimp b_dw) * conj(psi(a'_up + 2^Nimp b_up, a'_dw + 2^Nimp b_dw)),
 *   io = a_up + 2^Nimp a_dw, jo = a'_up + 2^Nimp a'_dw  (0-based; :539-562: impurity bits low, bath bits high).
 * hxv_cluster_dm_elems: the length of cdm in doubles, 2 * 16^Nimp: complex(8), interleaved, in the reference's Fortran order, element
 * (io,jo) at 2*(io + 4^Nimp*jo); 0 for handles without basis maps (from CSR), dw panels and Nimp > 5.
 * hxv_cluster_dm_accumulate: d_psi is a device vector of h (this rank's slab in the padded layout, device row order included; pad rows are
 * never read).  accumulate == 0 overwrites cdm, otherwise adds weight * (this state's matrix) to it; weight is the reference's peso
 * (:502-503).  Runs on the handle's stream and returns once the result is on the host.  The same vector on the same handle gives the same
 * bits on every call (no floating-point atomics).  Split sectors (after hxv_comm_init / _init_local): collective, every rank returns the
 * GLOBAL matrix (the reference computes it on the MPI master alone, :511), and all ranks fail together.  Errors: HXV_ERR_ARG for NULL
 * arguments; HXV_ERR_STATE for a handle without basis maps (from CSR, a dw panel) and for a split sector without its communicator;
 * HXV_ERR_UNSUPPORTED for Nimp > 5 (the dense matrix is 16 MB at Nimp 5 and 268 MB at Nimp 6).                                      */
int64_t hxv_cluster_dm_elems(const hxv_handle *h);
int hxv_cluster_dm_accumulate(hxv_handle *h, const void *d_psi, double weight, int32_t accumulate, double *cdm /* host */);

/* ---- reduced density matrix of a subset of the impurity orbitals, of device-resident states -----------------------------------
 * ED_IO/get_reduced_dm.f90 ed_get_reduced_density_matrix_single (:68-212): rho_S = Tr_env |psi><psi|, S the Nred impurity orbitals named by
 * orbital_mask, env everything else (the bath and the traced impurity orbitals).  The reference traces the dense cluster_density_matrix;
 * this entry works from the vector, so there is no limit on Nimp (the cluster matrix above ends at Nimp 5):
 *   rdm(io,jo) += weight * sum over (e_up,e_dw) of sg(i) sg(j) psi(a_up|e_up, a_dw|e_dw) * conj(psi(a'_up|e_up, a'_dw|e_dw)),
 *   io = a_up + 2^Nred a_dw, jo = a'_up + 2^Nred a'_dw  (0-based), a = the occupations of the masked orbitals in ascending orbital order
 *   (the reference's bjoin of state(red_indices), :193-210 and :146-147).
 * orbital_mask: bit b is set when the impurity orbital whose bit in a spin configuration is b belongs to S; the reference's
 *   b = jorb + (ilat-1)*Norb - 1 of orbital_mask(ilat,jorb) (:115), the low Nimp bits the cluster matrix indexes.  1 <= Nred <= 4.
 * fermi_sign 0: sg = +1, the plain partial trace.  These are the reference's numbers: its get_sign (:170-191) zeroes the reduced orbitals
 *   before it counts, the loop keeps pairs with equal traced bits (:145), so IsignUP*IsignDW*JsignUP*JsignDW (:148) is +1 for every pair that
 *   contributes.  The spectrum of this matrix is physical for some subsets only: on Slater determinants of a four-orbital cluster the
 *   entropy of S = {0,1} and {1,2,3} equals the closed form, that of S = {0,2} and {0,3} misses it by 2e-2 to 2.6e-1.
 * fermi_sign 1: sg(i) = (-1)^n, n = for every occupied orbital r of S the number of occupied orbitals outside S below r, per spin: the
 *   Jordan-Wigner string.  This matrix is the one whose spectrum (entanglement entropy, purity) is physical for any subset.
 * hxv_reduced_dm_elems: the length of rdm in doubles, 2 * 16^Nred: complex(8), interleaved, Fortran order, element (io,jo) at
 * 2*(io + 4^Nred*jo); Hermitian, the lower triangle filled by conjugation, the diagonal's imaginary part exactly 0.  0 for handles without
 * basis maps, dw panels, an empty mask, a mask outside the Nimp bits and Nred > 4.
 * hxv_reduced_dm_accumulate: d_psi, weight, accumulate, the stream, determinism (no floating-point atomics) and split sectors (collective,
 * every rank returns the GLOBAL matrix, all ranks fail together) as hxv_cluster_dm_accumulate; weight * raw is rounded before the add, so
 * an accumulated matrix equals the sum of the single results bit for bit.  The group tables of a (mask, fermi_sign) are built on first use
 * and kept with the sector image, the last few of them.  Errors: HXV_ERR_ARG for NULL arguments, an empty mask, a mask outside the
 * impurity bits and fermi_sign not 0 or 1; HXV_ERR_UNSUPPORTED for Nred > 4; HXV_ERR_STATE for a handle without basis maps (from CSR, a dw
 * panel) and for a split sector without its communicator.                                                                           */
int64_t hxv_reduced_dm_elems(const hxv_handle *h, uint32_t orbital_mask);
int hxv_reduced_dm_accumulate(hxv_handle *h, const void *d_psi, uint32_t orbital_mask, int32_t fermi_sign, double weight, int32_t accumulate,
                              double *rdm /* host */);

/* ---- density-type operators on device-resident states: the start vectors of the spin and charge susceptibilities ---------------
 * The two-particle stage of the reference (buildChi_impurity, ED_GREENS_FUNCTIONS.f90:68-106: spinChi, densChi) starts from O|psi> with
 * O diagonal in the Fock basis.  For nops operators  O_a = sum_is (cu_a[is] n_is,up + cd_a[is] n_is,dw)  over the Nimp impurity orbitals
 * (is = iorb + ilat*Norb, 0-based: the low Nimp bits of each spin's configuration, as in hxv_observables_accumulate) this entry computes
 *     out_a = (f_a - m_a) psi  element by element,   f_a(iup,idw) = sum_is cu_a[is] bit_is(up configuration) + cd_a[is] bit_is(dw configuration),
 *     mean[a]  = <psi|O_a|psi> / <psi|psi>   (always returned),    m_a = mean[a] if subtract_mean != 0, else 0,
 *     norm2[a] = <out_a|out_a>.
 * S^z_i is cu = +1/2, cd = -1/2 on orbital i; n_i is cu = cd = 1; totals and staggered sums are further rows of coef.  With subtract_mean
 * the outputs are the fluctuations dO_a|psi>: the start vector AND the probes of hxv_lanczos_tridiag_probes for
 *     chi_ab(z) = - sum_n [ w_n[a] / (z - e_n) - conj(w_n[a]) / (z + e_n) ],   e_n = poles[n] - E,
 * w_n[a] the weights hxv_gf_from_probes returns for the run started from out_b with the probes out_a and norm = sqrt(norm2[b]), E the
 * energy of psi (INTEGRATION.md section 4 has the call order, the thermal sum and the cutoff that drops the rounding ghosts of psi at e_n = 0).
 *   coef    : host, [nops][2][Nimp] doubles: for every operator cu[0..Nimp) then cd[0..Nimp).
 *   d_psi   : a device vector of h (this rank's slab in the padded layout, device row order included); pad rows are never read; unchanged.
 *   d_out   : host list of nops device vectors of h, all different and none of them d_psi; every element is written, pad rows as zero.
 * Two passes: the first reads psi once for all operators (the nops + 1 sums), the second reads it once more, writes the nops vectors and
 * sums their norms: 16 + (16 + 16 nops) bytes per basis state.  A diagonal operator keeps the row and the basis sign of a device row
 * cancels, so a device row order only changes where the occupations are looked up.  No floating-point atomics and a fixed work list: the
 * same inputs on the same handle give the same bits on every call.  The scratch (a few KB) comes from the device-buffer cache and goes back
 * before the call returns; the occupation words are built on first use and kept with the sector image.  Runs on the handle's stream and
 * returns when the scalars are on the host.
 * SPLIT SECTORS (after hxv_comm_init / hxv_comm_init_local): collective; d_psi and the outputs are this rank's slabs; the nops + 1 sums of
 * the first pass travel in ONE all-reduce, the nops norms of the second in ONE more, and every rank returns the global numbers.  A failure
 * of one rank's own arguments or resources is agreed on before the first collective step: every rank returns an error, nobody waits.
 * Errors (nothing is written): HXV_ERR_ARG for NULL arguments, nops outside [1, HXV_MAX_DENSITY_OPS], a NULL or repeated output, an output
 * equal to d_psi, a coefficient that is not finite, a state that is zero or not finite; HXV_ERR_STATE for handles without basis maps (from
 * CSR, dw panels) and for a split sector without its communicator; HXV_ERR_UNSUPPORTED for Nimp > 10.                                  */
#define HXV_MAX_DENSITY_OPS 8
int hxv_apply_density_ops(hxv_handle *h, int32_t nops, const double *coef /* [nops][2][Nimp]: cu then cd, is = iorb + ilat*Norb */,
                          int32_t subtract_mean, const void *d_psi, void *const *d_out /* nops device vectors of h */,
                          double *mean /* [nops] */, double *norm2 /* [nops] */);

/* ---- operators that change both spin sectors at once: the start vectors of the pair and spin-flip susceptibilities ---------------
 * The third susceptibility of the reference's two-particle stage (build_chi_pair, ED_GREENS_FUNCTIONS.f90:68-106, carried commented out)
 * and the transverse spin susceptibility <<S^-;S^+>> start from O|psi> with
 *     d_out = sum_t coef_t X_t Y_t d_psi,   X_t = c^dagger (create_up = 1) or c (0) on orbital orb_up[t] of spin up,
 *                                           Y_t = c^dagger (create_dw = 1) or c (0) on orbital orb_dw[t] of spin dw,
 * the two flags the same for all terms: c_{i,up} c_{j,dw} reaches (nup-1, ndw-1), c^+_{j,dw} c_{i,up} reaches (nup-1, ndw+1).  Orbitals are
 * 0-based in [0, Ns) as in hxv_apply_ladder (bath orbitals included); `to` is the sector (nup +- 1, ndw +- 1) the flags name, same Ns, same
 * device.  The terms are summed in the order given; a repeated (i, j) pair is allowed.  *norm2 = <out|out>; norm2 may be NULL.
 * SIGN CONVENTION: that of two successive hxv_apply_ladder calls, each with its same-spin sign (-1)^(occupied orbitals of the SAME spin
 * below the orbital) and no cross-spin sign; under it X_t and Y_t commute, and a single term with coef = 1 equals either order of the two
 * ladder calls through the intermediate sector bit for bit (an element no term reaches is +0 here; the second ladder call may leave -0 there,
 * differently in its two orders).  This differs from the true fermionic product by ONE constant +-1 per pair of
 * sectors ((-1)^nup for an operator that moves a dw particle past all the up ones), which cancels in every <psi|O_a ... O_b^+|psi>.
 * LAYOUT: d_psi is a vector of `from`, d_out one of `to`, both in the padded device layout; pad rows of d_psi are never read, every element
 * of d_out is written, pad rows as exact zeros; d_out != d_psi.  DEVICE ROW ORDER: the row changes anyway, so each side's own order and
 * basis signs apply and -- unlike a spin-dw ladder -- the two sectors need not share an order: the result equals hxv_vector_to_host / host
 * arithmetic / hxv_vector_from_host whether none, one or both sectors have an order.
 * One gather pass over the target: a thread owns elements of one target column, so the source column of a term is uniform over a workgroup
 * and a term that does not reach the column is skipped for all of it; every distinct up orbital is looked up once per row for all the terms
 * that use it; one 16-byte store per element; <out|out> from per-workgroup partial sums added in a fixed order.  A real d_psi with real
 * coefficients gives imaginary parts that are exactly zero.  No floating-point atomics: the same inputs on the same handles give the same
 * bits on every call.  The tables -- per distinct up orbital: target device row -> source device row and sign; per distinct dw orbital:
 * target column -> source column and sign -- are built on first use and kept with `to`'s sector image, by source sector, flags and orbital.
 * Runs on `to`'s stream and returns when norm2 is on the host.
 * SPLIT SECTORS ARE NOT BUILT: HXV_ERR_UNSUPPORTED when either handle has nranks > 1, decided locally and identically on every rank before
 * any collective step.
 * Errors (nothing is written): HXV_ERR_ARG for a NULL handle, vector or term array, nterms outside [1, HXV_MAX_SPIN_PAIR_TERMS], an orbital
 * outside [0, Ns), a coefficient that is not finite, d_out == d_psi, handles on different devices or with different Ns, `to` not the sector
 * the flags name; HXV_ERR_STATE for handles without basis maps (from CSR, dw panels); HXV_ERR_UNSUPPORTED as above.                    */
#define HXV_MAX_SPIN_PAIR_TERMS 32
int hxv_apply_spin_pair(hxv_handle *from, hxv_handle *to, int32_t create_up, int32_t create_dw, int32_t nterms, const int32_t *orb_up,
                        const int32_t *orb_dw, const double *coef /* [nterms] complex, interleaved */, const void *d_psi, void *d_out,
                        double *norm2);

/* ---- one-body operators inside a sector: bond, current, exciton susceptibilities, one-body density matrix -----------------
 * O = sum_t coef_t c^dagger_{i_t s_t} c_{j_t s_t}: the particle-conserving same-spin bilinears, which stay inside the handle's sector.
 * spin 0 = up, 1 = dw; orb_to = i and orb_from = j are 0-based in [0, Ns), bath included, as in hxv_apply_ladder; i == j is allowed and
 * is the occupation of any orbital.  The bond operator B_ij = sum_s (c^+_is c_js + h.c.), the current J_ij = i sum_s (c^+_is c_js - h.c.)
 * and the inter-orbital excitons sum_s c^+_as c_bs (singlet), sum_s s c^+_as c_bs (triplet z) are term lists of this kind (the triplet xy
 * component c^+_a,up c_b,dw is hxv_apply_spin_pair's).
 *   mean  = <psi|O|psi> / <psi|psi>, complex (re, im), always returned;   d_out = (O - m) psi, m = mean when subtract_mean != 0, else 0;
 *   *norm2 = <out|out>.  mean and norm2 may each be NULL.  Terms are summed in the order given; a repeated (spin, i, j) is allowed.
 * SIGN: the true fermionic one, (-1)^(occupied same-spin orbitals strictly between i and j) -- the product of the signs of c_j then
 * c^dagger_i as hxv_apply_ladder applies them; a same-spin bilinear carries no cross-spin sign.  A single term with coef = 1 and
 * subtract_mean = 0 equals the two ladder calls through (nup-1, ndw) or (nup, ndw-1) bit for bit, except that an element no term reaches
 * is +0 here and may be -0 there.
 * LAYOUT: d_psi and d_out are vectors of `h` in the padded device layout; pad rows of d_psi are never read, every element of d_out is
 * written, pad rows as exact zeros; d_out != d_psi.  DEVICE ROW ORDER: the handle's own on both sides; the up tables are by device row and
 * carry the basis signs of source and target row, so the host result is the same bit for bit with or without an order.  A real d_psi with
 * real coefficients gives imaginary parts that are exactly zero.
 * One gather pass: a work item is 256 rows of one column; a dw term reads the same rows of another column (its table entry is uniform
 * over the workgroup, a dead column skips the term), an up term gathers another row of the same column, each distinct up table looked up
 * once per row; the first live term is stored, the others added in order; one 16-byte store per element.  <psi|psi>, <psi|out> and
 * <out|out> ride along as per-workgroup partial sums added in a fixed order.  With subtract_mean a streaming pass computes out -= m psi
 * and sums <out|out> afresh from what it stores (not norm2 - |m|^2 <psi|psi>, which cancels for near-eigen-operators).  No floating-point
 * atomics, a fixed work list: the same inputs on the same handle give the same bits on every call.  Per-call scratch (the partial sums)
 * comes from the buffer cache and is back when the call returns.  Runs on the handle's stream and returns when the scalars are on the
 * host; nothing Dim-sized crosses PCIe.
 * TABLES: one per distinct (spin, i, j), 4 dim_s bytes, built on first use and kept with the handle's sector image; an image keeps at most
 * 128 of them (C3: 6.6 MB; Ns = 18 at half filling: 25 MB -- all 2 Ns^2 would be 126 MB there), the least recently used one goes first.
 * SPLIT SECTORS ARE NOT BUILT: HXV_ERR_UNSUPPORTED when the handle has nranks > 1, decided locally and identically on every rank before
 * any collective step (up terms are rank-local, dw terms need the exchanged vector).
 * Errors (nothing is written): HXV_ERR_ARG for a NULL handle, vector or array, nterms outside [1, HXV_MAX_ONE_BODY_TERMS], a spin that is
 * not 0 or 1, an orbital outside [0, Ns), a coefficient that is not finite, d_out == d_psi; HXV_ERR_STATE for handles without basis maps
 * (from CSR, dw panels); HXV_ERR_UNSUPPORTED as above.  HXV_ERR_ARG also for a state that is zero or not finite: <psi|psi> is known only
 * from the gather pass, so in this one case d_out has been overwritten (mean and norm2 have not).                                      */
#define HXV_MAX_ONE_BODY_TERMS 32
int hxv_apply_one_body(hxv_handle *h, int32_t nterms, const int32_t *spin /* 0 up, 1 dw */, const int32_t *orb_to /* i */,
                       const int32_t *orb_from /* j */, const double *coef /* [nterms] complex, interleaved */, int32_t subtract_mean,
                       const void *d_psi, void *d_out, double *mean /* [2] re, im */, double *norm2);

/* ---- device vectors owned by the library --------------------------------------------------------------------------------
 * For host programs without a HIP binding of their own (the Fortran glue): a local vector of the handle's sector in the padded device
 * layout (hxv_localvec_elems() complex elements, zeroed), from the engine's buffer cache.  Such a pointer is what the device drivers take
 * and return (hxv_lanczos_eigh's d_vect, hxv_apply_ladder's d_psi / d_out, hxv_lanczos_tridiag's d_vin), so a Green's-function channel --
 * ground state, c^dagger|gs>, tridiagonalisation (ED_GF_NORMAL.f90:174-217) -- runs without a Dim-sized PCIe transfer; the two copies
 * convert to / from the reference's contiguous host layout when a vector is wanted on the host after all.  hxv_vector_free takes the handle the
 * vector was allocated on, BEFORE that handle is destroyed; hxv_destroy returns whatever was not freed.                              */
int hxv_vector_alloc(hxv_handle *h, void **d_vec);
int hxv_vector_alloc_many(hxv_handle *h, int32_t count, void **d_vec); /* `count` vectors in one allocation, hxv_localvec_elems() apart: the d_evecs of hxv_eigh_lowest; freed as one */
int hxv_vector_free(hxv_handle *h, void *d_vec);
int hxv_vector_from_host(hxv_handle *h, const void *v_host, void *d_vec); /* writes every element of d_vec: pad rows zero, whatever it held */
int hxv_vector_to_host(hxv_handle *h, const void *d_vec, void *v_host);

/* ---- device-buffer cache.  A fresh hipMalloc costs ~25 ms per GB on this platform (0.7 s for the 28 GB Krylov basis of
 * hxv_eigh_lowest at Ns=16), and an ED run opens sectors one after another, so the vector-sized buffers a handle frees
 * (dw-hop scratch, Lanczos vectors, staging, Krylov basis) are kept per device and reused by the next handle.
 * Environment: HXV_POOL=0 disables it, HXV_POOL_MAX_GB caps the cached bytes (default 40 % of the device memory).
 * hxv_pool_trim returns everything cached on `device` (all devices if < 0) to the driver.                        */
int hxv_pool_trim(int32_t device);
int hxv_pool_stats(int32_t device, int64_t *cached_bytes, int64_t *hits, int64_t *misses);

/* ---- sector-image cache.  The reference opens and closes a sector around EVERY Lanczos run: once per sector in ED_DIAG.f90:142-186 and
 * once per Green's-function channel in ED_GF_NORMAL.f90:208-222 (+7 siblings; 56 channels of a 2x2 cluster re-open the same four sectors
 * N+-1).  What hxv_create_from_model builds -- basis maps, one-spin matrices, tile plan, ~50 device tables -- depends only on the model
 * bytes, (nup, ndw), (rank, nranks), the exchange and the device; the engine keeps the images of closed sectors and a re-open with the
 * same inputs shares them (identical products bit for bit; a different bath is a different key).  Environment: HXV_SECTOR_CACHE=0 disables
 * it, HXV_SECTOR_CACHE_MB caps host + device bytes in whole MiB (a fraction is dropped: 0.5 is 0, nothing is kept; default 2048, least
 * recently used out first).  hxv_get_option(h, "open_cache_hit" | "open_us_host" | "open_us_plan" | "open_us_upload" | "open_us_total")
 * tells what THIS open cost.  Handles from hxv_create_from_csr and panel handles are not cached.                                */
int hxv_sector_cache_clear(void);
int hxv_sector_cache_stats(int64_t *entries, int64_t *bytes, int64_t *hits, int64_t *misses); /* any out may be NULL */

/* Handles created (hxv_create_*; the internal row-panel handle of an exchange-mode-2 sector counts too) and not yet destroyed, process-wide:
 * what a host program's leak check reads after its last delete_Hv_sector (the Fortran demo asserts 0 after its lifetime cases).            */
int64_t hxv_live_handles(void);

/* ---- introspection (parity tests against spH0ups/spH0dws/spH0d) ------------------------ */
int hxv_get_maps(const hxv_handle *h, int32_t *map_up, int32_t *map_dw); /* Hs(1)%map, Hs(2)%map */
int64_t hxv_nnz(const hxv_handle *h, int32_t which);                      /* 0: H_up, 1: H_dw */
/* CSR of the one-spin matrix in the reference's row-list order; cols 1-based */
int hxv_get_csr(const hxv_handle *h, int32_t which, int64_t *rowptr, int32_t *cols, double *vals);
/* local diagonal (vecdim doubles; the engine requires a real diagonal) */
int hxv_get_diag(const hxv_handle *h, double *diag);

/* Options (name, value), in three groups.  A maintainer needs group 1 only.
 *
 * 1. BEHAVIOUR (what the engine computes or which algorithm runs; results stay within the stated tolerances)
 *   "kernel"            1 = tiled two-pass kernels [default], 0 = one thread per element (cross-check / fallback)
 *   "real_vectors"      1 [default] = device Lanczos drivers run on real vectors when H and the start vector are real
 *   "lanczos_fused"     1 [default] = recurrence fused into the product's epilogue; 0 = separate vector kernels
 *   "lanczos_graph"     1 [default] = fixed-length tridiagonalisations run device-only, three iterations per hipGraph
 *   "lanczos_inplace"   1 [default] = on a split sector the device Lanczos vectors live in their slot of a gather buffer (three full-size
 *                       buffers per rank instead of one plus three slabs; no slab copy per product; same numbers bit for bit);
 *                       get "slab_copies" counts the exchanges that had to copy
 *   "eigh_degenerate"   0 [default] = one Krylov space like ARPACK; 1 = hxv_eigh_lowest locks the converged pairs and looks for further copies of
 *                       degenerate levels (C3: +60 products on 380; at worst as many again)
 *   "eigh_measure_all"  0 [default] = partial re-orthogonalisation (loss of orthogonality estimated by the omega recurrence, whole-basis
 *                       Gram-Schmidt only when needed); 1 = every projection measured at every step
 *   "eigh_keep_pct"     5..80 [20]: share of the Krylov basis beyond the wanted pairs that a thick restart of hxv_eigh_lowest keeps
 *   "eigh_fuse_restart" 1 [default] = the restart rotation also measures the residual vector, the first step of a cycle removes the arrow and
 *                       measures in one pass; 0 = separate passes (same algorithm)
 *   "fold_nd"           1 [default] = spH0nd inside pass A; 0 = as its own pass over Hv
 *   "exchange_overlap"  0 [default] | 1: exchange mode 2 of a split sector runs diagonal + up hops on a second stream WHILE the two transposes and
 *                       the panel product are under way (the reference's order, ED_HAMILTONIAN_SPARSE_HxV.f90:250-296) and adds the dw part at the
 *                       end; plain products only; 32 B per local state more HBM traffic, for hiding pass A behind the links
 *
 * 2. TILE SHAPE AND SCHEDULING (results unchanged up to summation order; changing a shape rebuilds a handle-private plan, the shared sector image
 *    keeps the default one; invalid combinations are refused with a message)
 *   "cols_per_tile" 2|4|8 [4; complex vectors use at most 4 per tile], "rows_per_tile" 0|2|4|8 [0 = 4, or 8 for sectors whose row panels exceed
 *   the L2], "lds_budget_kb[_up|_dw]" 8..144 [64], "threads_up|_dw" 256|512|1024 [1024], "sort_mode" 0..2 [0], "sort_mode_dw" 0|1 [1],
 *   "wt_cols" 2|4|8|16 [4], "tile_bits_up|_dw" (force the block bits), "lds_min_kb_up|_dw", "spread_banks" 0|1 [1].
 *   Pass A as pipelined jobs (LDS-DMA tile ring, one workgroup per CU): "job_up" 2 [default: for the fused Lanczos product only] |
 *   1 (always) | 0 (one tile per workgroup), "job_groups" columns per job [about 100], "job_cols" 1, "job_stages" ring depth 2..8 [4],
 *   "job_max_blocks" [32].  The engine falls back to the one-tile kernels where jobs do not apply (real vectors, stored diagonal, more than
 *   24 in-block entries per row, more than 8 out-of-block partners -- row slots plus block hops -- of a block, blocks over 960 rows;
 *   get "job_up_active" tells whether a plain product with "job_up" = 1 runs as jobs).
 *   "wt_colmajor" 0|1 [1: the blocked dw-hop scratch holds column-major patches -- pass A's accumulator init reads R*16 contiguous bytes per column
 *   and patch instead of every lane its own 64-byte stretch; bit-identical],
 *   "real_dw_pairs" 0|1 [1: pass B of the REAL-vector product runs the complex kernel on pairs of rows -- one table decode and one 16-byte LDS
 *   gather per two elements, bit-identical],
 *   "pair_rows" -1|0|1 [-1 = by sector size: pass B runs the two row groups of a 128-byte line back to back],
 *   "block_order" -1|0|1|2 [-1: dispatch order of a group's blocks -- 1 by the particle number of the high orbitals (coupled blocks close
 *   together; the automatic choice where table classes are few), 0 largest block first, 2 natural].
 *
 * 3. TIMING EXPERIMENTS (results are wrong or partial when set; refused unless HXV_EXPERIMENTS=1 is in the environment)
 *   "passes" 1|2|3 [3], "debug" bit mask, "job_debug" bit mask.
 *   Two bits of the debug mask leave the results bit-identical (same gate): 4096, pass B issues its loads also for the pair iterations no
 *   lane of a wave owns (the kernel without the dead-wave skip, for A/B timings); 8192, pass B runs its phases in the earlier order
 *   (out-of-block hops after the in-block ones, their sums added into the LDS tile) also where the plan allows the out-of-block sums in
 *   registers.
 *
 * hxv_get_option additionally reports plan statistics ("tile_bits_up", "nblocks_up", "slots_in_up_x100", "max_outer_up", "ncoef_up" / "ncoef_dw" (distinct hopping amplitudes), "job_up_active", ...),
 * driver read-backs ("pass_b_order_last": the phase order the last pass-B launch ran, 1 = out-of-block sums in registers, 0 = the earlier
 * order [eight pairs per thread, row-major scratch patches, a largest block that leaves no room for wt_cols - 1 dead columns, debug bit 8192],
 * -1 = no launch since the plan was made; "lanczos_real_last", "eigh_last_full_passes", "eigh_last_local_passes", "eigh_last_search_products",
 * "eigh_last_check_products", "slab_copies", "allreduce_count" (the sum all-reduces a split sector's drivers have made on this handle), "pool_live_blocks" (the blocks of the
 * device-buffer cache that are handed out on the handle's DEVICE and not yet returned -- every handle's vectors and work buffers and whatever a
 * driver call under way holds; a driver call leaves it where it found it, however it returns); which restart code the last hxv_eigh_lowest ran: "eigh_last_restarts" thick restarts of the search
 * round, "eigh_last_fused_restarts" those whose rotation also measured the residual vector, "eigh_last_fused_first_steps" restart cycles whose
 * first step removed the arrow and measured in one pass) and what the open cost ("open_cache_hit", "open_us_host|plan|upload|total").
 * Every option of groups 1 and 2 reads back the value hxv_set_option stored ("tile_bits_up|_dw": the block bits of the plan in use;
 * "rows_per_tile" 0: the 4 or 8 it resolved to; "lds_budget_kb": through its "_up" / "_dw" halves); -1 is the answer to an unknown name. */
int hxv_set_option(hxv_handle *h, const char *name, int64_t value);
int64_t hxv_get_option(const hxv_handle *h, const char *name);

typedef struct {
  int64_t n_apply;          /* products since creation                     */
  int64_t algorithmic_bytes; /* 32 B x local rows per product   */
  int64_t device_bytes;     /* bytes of device memory held by the handle   */
  int32_t kernel;           /* active kernel variant                       */
  int32_t real_h;           /* 1 if all hopping amplitudes are real        */
  int32_t k_up, k_dw;       /* max stored entries per row of H_up / H_dw   */
  int32_t n_hops_up, n_hops_dw;
  int64_t h2d_bytes;        /* vector-sized host -> device traffic of the host-array entry points (hxv_apply_host, *_host drivers,   */
  int64_t d2h_bytes;        /* hxv_vector_from_host) and device -> host (results, hxv_vector_to_host) since creation: 0 + 0 for a    */
                            /* Green's-function channel that runs device-resident                                                  */
} hxv_stats;
int hxv_get_stats(const hxv_handle *h, hxv_stats *out);

/* last error message of the calling thread ("" if none) */
const char *hxv_last_error(void);
/* library version string */
const char *hxv_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HXV_H */
