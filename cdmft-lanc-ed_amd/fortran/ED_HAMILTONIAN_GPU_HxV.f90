!> ISO_C_BINDING glue between the reference's Fortran host and the HIP engine (include/hxv.h).
!!
!! It provides a module procedure with EXACTLY the abstract interface cc_sparse_HxV
!! (ED_VARS_GLOBAL.f90:72-78), so that the reference's pointer can be bound to it,
!!     spHtimesV_p => gpuMatVec_main            (ED_HAMILTONIAN.f90:129-141)
!! and ED_DIAG / ED_GF_NORMAL (the SciFortran Lanczos callers) stay untouched, plus the
!! open/close hooks that build_Hv_sector / delete_Hv_sector call (ED_HAMILTONIAN.f90:39-190).
!! Errors follow the reference's convention: a non-zero status from the C side becomes `stop`.
!! INTEGRATION.md shows the few lines added to ED_HAMILTONIAN.f90.
module ED_HAMILTONIAN_GPU_HXV
  use, intrinsic :: iso_c_binding
  implicit none
  private

  public :: gpu_build_Hv_sector
  public :: gpu_delete_Hv_sector
  public :: gpu_vecDim_Hv_sector
  public :: gpuMatVec_main
  public :: gpuMatVec_MPI_main
  public :: gpu_comm_unique_id
  public :: gpu_comm_init
  !sp_eigh's replacement can look for hidden copies of degenerate levels (engine option "eigh_degenerate", include/hxv.h).  THIS GLUE ASKS FOR
  !THEM BY DEFAULT (ADVICE r5): it is the drop-in path that feeds es_add_state, ED_DIAG.f90:234-244 keeps every state within gs_threshold of
  !the minimum, and a 2x2 plaquette (point group D4) has degenerate levels inside a sector -- losing a copy gives a symmetry-broken G.  It
  !costs the check rounds (C3: 60 products on 380).  Set .false. BEFORE build_Hv_sector for exactly what ARPACK does (one Krylov space, no
  !extra products; the raw C-ABI's default).
  logical,public,save :: gpu_eigh_degenerate=.true.
  public :: gpu_lanc_tridiag_host
  public :: gpu_sp_lanc_tridiag
  public :: gpu_sp_lanc_tridiag_pair
  public :: gpu_sp_lanc_eigh
  public :: gpu_sp_eigh
  !device-resident Green's-function pipeline (nothing Dim-sized crosses PCIe): see the block comment above gpu_sp_lanc_eigh_dev
  public :: gpu_vector
  public :: gpu_sp_lanc_eigh_dev
  public :: gpu_sp_eigh_dev
  public :: gpu_keep_sector
  public :: gpu_apply_ladder
  public :: gpu_twin_vector
  public :: gpu_sp_lanc_tridiag_dev
  public :: gpu_sp_lanc_tridiag_pair_dev
  !off-diagonal Green's functions from one run per orbital (include/hxv.h: hxv_lanczos_tridiag_probes, hxv_gf_from_probes)
  public :: gpu_sp_lanc_tridiag_probes_dev
  public :: gpu_gf_from_probes
  !two probe runs on one product (real H; include/hxv.h: hxv_lanczos_tridiag_pair_probes)
  public :: gpu_sp_lanc_tridiag_pair_probes_dev
  public :: gpu_apply_density_ops_dev
  public :: gpu_apply_spin_pair_dev
  public :: gpu_apply_one_body_dev
  !Chebyshev recurrence: moments and f(H) on a device-resident state (include/hxv.h: hxv_chebyshev_moments, hxv_chebyshev_apply)
  public :: gpu_chebyshev_moments_dev
  public :: gpu_chebyshev_apply_dev
  !the same on real vectors (real H, real start vector and probes), and the seeded random device state they start from
  public :: gpu_chebyshev_moments_real_dev
  public :: gpu_chebyshev_apply_real_dev
  public :: gpu_vector_random_dev
  public :: gpu_vector_to_host
  public :: gpu_vector_from_host
  public :: gpu_free_vector
  public :: gpu_pcie_bytes
  public :: gpu_live_sectors
  !the reference's own stored matrices handed over (spH0ups(1), spH0dws(1), spH0d, spH0nd flattened to CSR)
  public :: gpu_build_Hv_sector_from_csr
  public :: gpu_set_nonlocal_csr
  !what the engine built for the open sector, in the layout gpu_build_Hv_sector_from_csr takes (parity against spH0ups / spH0dws / spH0d)
  public :: gpu_sector_nnz
  public :: gpu_get_sector_csr
  public :: gpu_get_sector_diag
  !impurity observables of device-resident states (ED_OBSERVABLES.f90 lanc_observables / lanc_local_energy / single-particle density matrix)
  public :: gpu_observables_dev
  public :: gpu_get_observables
  !cluster reduced density matrix of device-resident states (ED_OBSERVABLES.f90 density_matrix_impurity, cluster_density_matrix)
  public :: gpu_cluster_dm_dev
  public :: gpu_get_cluster_dm
  public :: gpu_reduced_dm_dev

  !> A vector that lives on the device, in the layout of the sector it was made for.  Opaque: pass it back to the gpu_* routines.
  type :: gpu_vector
     type(c_ptr) :: d      = c_null_ptr    !device buffer (include/hxv.h: hxv_vector_alloc)
     type(c_ptr) :: sector = c_null_ptr    !the sector (engine handle) it belongs to
     logical     :: owns_sector = .false.  !gpu_keep_sector was called with this vector (informational: the sector's life is counted, below)
     logical     :: view = .false.         !part of another vector's allocation (eigenvectors 2.. of gpu_sp_eigh_dev)
     type(c_ptr) :: base   = c_null_ptr    !the allocation it lives in (= d unless a view)
     integer(8)  :: sector_id = 0          !serial numbers of the sector and of the allocation in the lifetime tables below: addresses are
     integer(8)  :: alloc_id  = 0          !re-issued by malloc / the engine's buffer cache once freed, serials never (ADVICE r5)
  end type gpu_vector

  !Lifetimes are COUNTED, so vectors may be freed in any order (ADVICE r4): an allocation goes back to the engine when the last
  !gpu_vector in it is freed (the eigenvectors of gpu_sp_eigh_dev share one), and a kept sector (gpu_keep_sector) is closed when the last
  !vector made on it is freed -- whichever vector that is.  A sector closed by gpu_delete_Hv_sector while vectors of it are still alive
  !takes their memory with it (hxv_destroy returns it): those vectors become empty shells and freeing them later is a no-op.
  !Entries are identified by a SERIAL NUMBER taken when the sector is opened / the allocation is made, never by address: a sector closed by
  !gpu_delete_Hv_sector with live vectors keeps its (dead) entry until those shells are freed, and the next build_Hv_sector very likely gets
  !the same handle address -- matched by address, the new sector would inherit dead=.true. and leak (ADVICE r5).
  type :: ref_entry
     integer(8)  :: id   = 0
     integer     :: n    = 0
     logical     :: kept = .false.         !sectors: stays open until its last vector is freed
     logical     :: dead = .false.         !sectors: destroyed while vectors were alive
  end type ref_entry
  integer,parameter    :: MAXREF=512
  type(ref_entry),save :: sector_refs(MAXREF), alloc_refs(MAXREF)
  integer(8),save      :: next_serial=0      !last serial number handed out (sectors and allocations share the counter)
  integer(8),save      :: handle_serial=0    !serial of the OPEN sector (`handle`), 0: none

  !> SciFortran's drivers are generic in exactly this way: the serial form takes the product first, the MPI form the
  !! communicator first (call sites ED_DIAG.f90:152-156,161-165,176-184; ED_GF_NORMAL.f90:215,217).  Both forms end in
  !! the same device driver: on a split sector the engine's own communicator (gpu_comm_init) does the all-reduces, so
  !! MpiComm is accepted for call compatibility only.
  interface gpu_sp_eigh
     module procedure gpu_sp_eigh_serial, gpu_sp_eigh_mpi
  end interface gpu_sp_eigh
  interface gpu_sp_lanc_eigh
     module procedure gpu_sp_lanc_eigh_serial, gpu_sp_lanc_eigh_mpi
  end interface gpu_sp_lanc_eigh
  interface gpu_sp_lanc_tridiag
     module procedure gpu_sp_lanc_tridiag_serial, gpu_sp_lanc_tridiag_mpi
  end interface gpu_sp_lanc_tridiag

  !> mirrors struct hxv_stats of include/hxv.h
  type, bind(C) :: hxv_stats
     integer(c_int64_t) :: n_apply, algorithmic_bytes, device_bytes
     integer(c_int32_t) :: kernel, real_h, k_up, k_dw, n_hops_up, n_hops_dw
     integer(c_int64_t) :: h2d_bytes, d2h_bytes
  end type hxv_stats

  !> mirrors struct hxv_model of include/hxv.h
  type, bind(C) :: hxv_model
     integer(c_int32_t) :: nlat, norb, nspin, nbath
     integer(c_int32_t) :: hfmode, reserved
     real(c_double)     :: uloc(5)
     real(c_double)     :: ust, jh, jx, jp, xmu
     type(c_ptr)        :: imphloc, hbath, vbath
  end type hxv_model

  interface
     integer(c_int) function hxv_create_from_model(model,nup,ndw,rank,nranks,device,out) bind(C,name="hxv_create_from_model")
       import :: c_int, c_int32_t, c_ptr, hxv_model
       type(hxv_model),intent(in)    :: model
       integer(c_int32_t),value      :: nup,ndw,rank,nranks,device
       type(c_ptr),intent(out)       :: out
     end function hxv_create_from_model
     integer(c_int) function hxv_set_option(h,name,value) bind(C,name="hxv_set_option")
       import :: c_ptr,c_int,c_char,c_int64_t
       type(c_ptr),value             :: h
       character(kind=c_char)        :: name(*)
       integer(c_int64_t),value      :: value
     end function hxv_set_option
     integer(c_int) function hxv_destroy(h) bind(C,name="hxv_destroy")
       import :: c_int, c_ptr
       type(c_ptr),value :: h
     end function hxv_destroy
     integer(c_int64_t) function hxv_live_handles() bind(C,name="hxv_live_handles")
       import :: c_int64_t
     end function hxv_live_handles
     integer(c_int64_t) function hxv_vecdim(h) bind(C,name="hxv_vecdim")
       import :: c_int64_t, c_ptr
       type(c_ptr),value :: h
     end function hxv_vecdim
     integer(c_int) function hxv_apply_host(h,nloc,v,hv) bind(C,name="hxv_apply_host")
       import :: c_int, c_int64_t, c_ptr, c_double_complex
       type(c_ptr),value                    :: h
       integer(c_int64_t),value             :: nloc
       complex(c_double_complex),intent(in) :: v(*)
       complex(c_double_complex)            :: hv(*)
     end function hxv_apply_host
     integer(c_int) function hxv_lanczos_tridiag_host(h,vin,nlanc,alanc,blanc,threshold,nsteps) bind(C,name="hxv_lanczos_tridiag_host")
       import :: c_int, c_int32_t, c_ptr, c_double, c_double_complex
       type(c_ptr),value                    :: h
       complex(c_double_complex),intent(in) :: vin(*)
       integer(c_int32_t),value             :: nlanc
       real(c_double)                       :: alanc(*),blanc(*)
       real(c_double),value                 :: threshold
       integer(c_int32_t)                   :: nsteps
     end function hxv_lanczos_tridiag_host
     integer(c_int) function hxv_lanczos_tridiag_pair_host(h,vin_a,vin_b,nlanc,alanc_a,blanc_a,alanc_b,blanc_b,threshold,nsteps_a,nsteps_b) &
          bind(C,name="hxv_lanczos_tridiag_pair_host")
       import :: c_int, c_int32_t, c_ptr, c_double, c_double_complex
       type(c_ptr),value                    :: h
       complex(c_double_complex),intent(in) :: vin_a(*),vin_b(*)
       integer(c_int32_t),value             :: nlanc
       real(c_double)                       :: alanc_a(*),blanc_a(*),alanc_b(*),blanc_b(*)
       real(c_double),value                 :: threshold
       integer(c_int32_t)                   :: nsteps_a,nsteps_b
     end function hxv_lanczos_tridiag_pair_host
     integer(c_int) function hxv_lanczos_eigh_host(h,nitermax,threshold,egs,vect,niter) bind(C,name="hxv_lanczos_eigh_host")
       import :: c_int, c_int32_t, c_ptr, c_double, c_double_complex
       type(c_ptr),value                    :: h
       integer(c_int32_t),value             :: nitermax
       real(c_double),value                 :: threshold
       real(c_double)                       :: egs
       complex(c_double_complex)            :: vect(*)
       integer(c_int32_t)                   :: niter
     end function hxv_lanczos_eigh_host
     integer(c_int) function hxv_eigh_lowest_host(h,neigen,ncv,maxrestart,tol,evals,evecs,nconv,nmatvec) bind(C,name="hxv_eigh_lowest_host")
       import :: c_int, c_int32_t, c_ptr, c_double, c_double_complex
       type(c_ptr),value                    :: h
       integer(c_int32_t),value             :: neigen,ncv,maxrestart
       real(c_double),value                 :: tol
       real(c_double)                       :: evals(*)
       complex(c_double_complex)            :: evecs(*)
       integer(c_int32_t)                   :: nconv,nmatvec
     end function hxv_eigh_lowest_host
     integer(c_int) function hxv_comm_unique_id(id) bind(C,name="hxv_comm_unique_id")
       import :: c_int, c_int8_t
       integer(c_int8_t) :: id(128)
     end function hxv_comm_unique_id
     integer(c_int) function hxv_comm_init(h,id) bind(C,name="hxv_comm_init")
       import :: c_int, c_int8_t, c_ptr
       type(c_ptr),value            :: h
       integer(c_int8_t),intent(in) :: id(128)
     end function hxv_comm_init
     integer(c_int) function hxv_create_from_csr(dimup,dimdw,up_rowptr,up_cols,up_vals,dw_rowptr,dw_cols,dw_vals,diag,rank,nranks,device,out) &
          bind(C,name="hxv_create_from_csr")
       import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double_complex
       integer(c_int32_t),value             :: dimup,dimdw,rank,nranks,device
       integer(c_int64_t),intent(in)        :: up_rowptr(*),dw_rowptr(*)
       integer(c_int32_t),intent(in)        :: up_cols(*),dw_cols(*)
       complex(c_double_complex),intent(in) :: up_vals(*),dw_vals(*),diag(*)
       type(c_ptr),intent(out)              :: out
     end function hxv_create_from_csr
     integer(c_int) function hxv_set_nonlocal_csr(h,rowptr,cols,vals) bind(C,name="hxv_set_nonlocal_csr")
       import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double_complex
       type(c_ptr),value                    :: h
       integer(c_int64_t),intent(in)        :: rowptr(*)
       integer(c_int32_t),intent(in)        :: cols(*)
       complex(c_double_complex),intent(in) :: vals(*)
     end function hxv_set_nonlocal_csr
     integer(c_int64_t) function hxv_nnz(h,which) bind(C,name="hxv_nnz")
       import :: c_int64_t, c_int32_t, c_ptr
       type(c_ptr),value        :: h
       integer(c_int32_t),value :: which
     end function hxv_nnz
     integer(c_int) function hxv_get_csr(h,which,rowptr,cols,vals) bind(C,name="hxv_get_csr")
       import :: c_int, c_int32_t, c_int64_t, c_ptr, c_double_complex
       type(c_ptr),value         :: h
       integer(c_int32_t),value  :: which
       integer(c_int64_t)        :: rowptr(*)
       integer(c_int32_t)        :: cols(*)
       complex(c_double_complex) :: vals(*)
     end function hxv_get_csr
     integer(c_int) function hxv_get_diag(h,diag) bind(C,name="hxv_get_diag")
       import :: c_int, c_ptr, c_double
       type(c_ptr),value :: h
       real(c_double)    :: diag(*)
     end function hxv_get_diag
     integer(c_int) function hxv_vector_alloc(h,d_vec) bind(C,name="hxv_vector_alloc")
       import :: c_int, c_ptr
       type(c_ptr),value       :: h
       type(c_ptr),intent(out) :: d_vec
     end function hxv_vector_alloc
     integer(c_int) function hxv_vector_alloc_many(h,count,d_vec) bind(C,name="hxv_vector_alloc_many")
       import :: c_int, c_int32_t, c_ptr
       type(c_ptr),value        :: h
       integer(c_int32_t),value :: count
       type(c_ptr),intent(out)  :: d_vec
     end function hxv_vector_alloc_many
     integer(c_int64_t) function hxv_localvec_elems(h) bind(C,name="hxv_localvec_elems")
       import :: c_int64_t, c_ptr
       type(c_ptr),value :: h
     end function hxv_localvec_elems
     integer(c_int) function hxv_eigh_lowest(h,neigen,ncv,maxrestart,tol,evals,d_evecs,nconv,nmatvec) bind(C,name="hxv_eigh_lowest")
       import :: c_int, c_int32_t, c_ptr, c_double
       type(c_ptr),value        :: h,d_evecs
       integer(c_int32_t),value :: neigen,ncv,maxrestart
       real(c_double),value     :: tol
       real(c_double)           :: evals(*)
       integer(c_int32_t)       :: nconv,nmatvec
     end function hxv_eigh_lowest
     integer(c_int) function hxv_vector_free(h,d_vec) bind(C,name="hxv_vector_free")
       import :: c_int, c_ptr
       type(c_ptr),value :: h,d_vec
     end function hxv_vector_free
     integer(c_int) function hxv_vector_from_host(h,v_host,d_vec) bind(C,name="hxv_vector_from_host")
       import :: c_int, c_ptr, c_double_complex
       type(c_ptr),value                    :: h,d_vec
       complex(c_double_complex),intent(in) :: v_host(*)
     end function hxv_vector_from_host
     integer(c_int) function hxv_vector_to_host(h,d_vec,v_host) bind(C,name="hxv_vector_to_host")
       import :: c_int, c_ptr, c_double_complex
       type(c_ptr),value         :: h,d_vec
       complex(c_double_complex) :: v_host(*)
     end function hxv_vector_to_host
     integer(c_int) function hxv_lanczos_eigh(h,nitermax,threshold,egs,d_vect,niter) bind(C,name="hxv_lanczos_eigh")
       import :: c_int, c_int32_t, c_ptr, c_double
       type(c_ptr),value        :: h,d_vect
       integer(c_int32_t),value :: nitermax
       real(c_double),value     :: threshold
       real(c_double)           :: egs
       integer(c_int32_t)       :: niter
     end function hxv_lanczos_eigh
     integer(c_int) function hxv_lanczos_tridiag(h,d_vin,nlanc,alanc,blanc,threshold,nsteps) bind(C,name="hxv_lanczos_tridiag")
       import :: c_int, c_int32_t, c_ptr, c_double
       type(c_ptr),value        :: h,d_vin
       integer(c_int32_t),value :: nlanc
       real(c_double)           :: alanc(*),blanc(*)
       real(c_double),value     :: threshold
       integer(c_int32_t)       :: nsteps
     end function hxv_lanczos_tridiag
     integer(c_int) function hxv_lanczos_tridiag_pair(h,d_vin_a,d_vin_b,nlanc,alanc_a,blanc_a,alanc_b,blanc_b,threshold,nsteps_a,nsteps_b) &
          bind(C,name="hxv_lanczos_tridiag_pair")
       import :: c_int, c_int32_t, c_ptr, c_double
       type(c_ptr),value        :: h,d_vin_a,d_vin_b
       integer(c_int32_t),value :: nlanc
       real(c_double)           :: alanc_a(*),blanc_a(*),alanc_b(*),blanc_b(*)
       real(c_double),value     :: threshold
       integer(c_int32_t)       :: nsteps_a,nsteps_b
     end function hxv_lanczos_tridiag_pair
     integer(c_int) function hxv_lanczos_tridiag_probes(h,d_vin,nprobes,d_probes,nlanc,alanc,blanc,overlaps,threshold,nsteps) &
          bind(C,name="hxv_lanczos_tridiag_probes")
       import :: c_int, c_int32_t, c_ptr, c_double, c_double_complex
       type(c_ptr),value         :: h,d_vin
       integer(c_int32_t),value  :: nprobes,nlanc
       type(c_ptr)               :: d_probes(*)
       real(c_double)            :: alanc(*),blanc(*)
       complex(c_double_complex) :: overlaps(*)
       real(c_double),value      :: threshold
       integer(c_int32_t)        :: nsteps
     end function hxv_lanczos_tridiag_probes
     integer(c_int) function hxv_lanczos_tridiag_pair_probes(h,d_vin_a,d_vin_b,nprobes,d_probes,nlanc,alanc_a,blanc_a,overlaps_a,&
          alanc_b,blanc_b,overlaps_b,threshold,nsteps_a,nsteps_b) bind(C,name="hxv_lanczos_tridiag_pair_probes")
       import :: c_int, c_int32_t, c_ptr, c_double, c_double_complex
       type(c_ptr),value         :: h,d_vin_a,d_vin_b
       integer(c_int32_t),value  :: nprobes,nlanc
       type(c_ptr)               :: d_probes(*)
       real(c_double)            :: alanc_a(*),blanc_a(*),alanc_b(*),blanc_b(*)
       complex(c_double_complex) :: overlaps_a(*),overlaps_b(*)
       real(c_double),value      :: threshold
       integer(c_int32_t)        :: nsteps_a,nsteps_b
     end function hxv_lanczos_tridiag_pair_probes
     integer(c_int) function hxv_gf_from_probes(nsteps,alanc,blanc,nprobes,overlaps,norm,poles,weights) bind(C,name="hxv_gf_from_probes")
       import :: c_int, c_int32_t, c_double, c_double_complex
       integer(c_int32_t),value  :: nsteps,nprobes
       real(c_double)            :: alanc(*),blanc(*),poles(*)
       complex(c_double_complex) :: overlaps(*),weights(*)
       real(c_double),value      :: norm
     end function hxv_gf_from_probes
     integer(c_int) function hxv_apply_ladder_axpy(from,to,orbital,spin,create,coef_re,coef_im,accumulate,d_psi,d_out,norm2) &
          bind(C,name="hxv_apply_ladder_axpy")
       import :: c_int, c_int32_t, c_ptr, c_double
       type(c_ptr),value        :: from,to,d_psi,d_out
       integer(c_int32_t),value :: orbital,spin,create,accumulate
       real(c_double),value     :: coef_re,coef_im
       real(c_double)           :: norm2
     end function hxv_apply_ladder_axpy
     integer(c_int) function hxv_twin_vector(from,to,d_psi,d_out) bind(C,name="hxv_twin_vector")
       import :: c_int, c_ptr
       type(c_ptr),value        :: from,to,d_psi,d_out
     end function hxv_twin_vector
     integer(c_int) function hxv_get_stats(h,st) bind(C,name="hxv_get_stats")
       import :: c_int, c_ptr, hxv_stats
       type(c_ptr),value :: h
       type(hxv_stats)   :: st
     end function hxv_get_stats
     type(c_ptr) function hxv_last_error() bind(C,name="hxv_last_error")
       import :: c_ptr
     end function hxv_last_error
     integer(c_int64_t) function hxv_obs_record_elems(h) bind(C,name="hxv_obs_record_elems")
       import :: c_int64_t, c_ptr
       type(c_ptr),value :: h
     end function hxv_obs_record_elems
     integer(c_int) function hxv_observables_accumulate(h,d_psi,weight,accumulate,record) bind(C,name="hxv_observables_accumulate")
       import :: c_int, c_int32_t, c_ptr, c_double
       type(c_ptr),value        :: h,d_psi
       real(c_double),value     :: weight
       integer(c_int32_t),value :: accumulate
       real(c_double)           :: record(*)
     end function hxv_observables_accumulate
     integer(c_int64_t) function hxv_obs_derived_elems(model) bind(C,name="hxv_obs_derived_elems")
       import :: c_int64_t, hxv_model
       type(hxv_model),intent(in) :: model
     end function hxv_obs_derived_elems
     integer(c_int) function hxv_observables_derive(model,record,out) bind(C,name="hxv_observables_derive")
       import :: c_int, c_double, hxv_model
       type(hxv_model),intent(in) :: model
       real(c_double),intent(in)  :: record(*)
       real(c_double)             :: out(*)
     end function hxv_observables_derive
     integer(c_int64_t) function hxv_cluster_dm_elems(h) bind(C,name="hxv_cluster_dm_elems")
       import :: c_int64_t, c_ptr
       type(c_ptr),value :: h
     end function hxv_cluster_dm_elems
     integer(c_int) function hxv_cluster_dm_accumulate(h,d_psi,weight,accumulate,cdm) bind(C,name="hxv_cluster_dm_accumulate")
       import :: c_int, c_int32_t, c_ptr, c_double
       type(c_ptr),value        :: h,d_psi
       real(c_double),value     :: weight
       integer(c_int32_t),value :: accumulate
       real(c_double)           :: cdm(*)
     end function hxv_cluster_dm_accumulate
     integer(c_int64_t) function hxv_reduced_dm_elems(h,orbital_mask) bind(C,name="hxv_reduced_dm_elems")
       import :: c_int64_t, c_int32_t, c_ptr
       type(c_ptr),value        :: h
       integer(c_int32_t),value :: orbital_mask   !uint32_t: the same 32 bits
     end function hxv_reduced_dm_elems
     integer(c_int) function hxv_reduced_dm_accumulate(h,d_psi,orbital_mask,fermi_sign,weight,accumulate,rdm) bind(C,name="hxv_reduced_dm_accumulate")
       import :: c_int, c_int32_t, c_ptr, c_double
       type(c_ptr),value        :: h,d_psi
       integer(c_int32_t),value :: orbital_mask,fermi_sign
       real(c_double),value     :: weight
       integer(c_int32_t),value :: accumulate
       real(c_double)           :: rdm(*)
     end function hxv_reduced_dm_accumulate
     integer(c_int) function hxv_apply_density_ops(h,nops,coef,subtract_mean,d_psi,d_out,mean,norm2) bind(C,name="hxv_apply_density_ops")
       import :: c_int, c_int32_t, c_ptr, c_double
       type(c_ptr),value         :: h,d_psi
       integer(c_int32_t),value  :: nops,subtract_mean
       real(c_double),intent(in) :: coef(*)
       type(c_ptr),intent(in)    :: d_out(*)
       real(c_double)            :: mean(*),norm2(*)
     end function hxv_apply_density_ops
     integer(c_int) function hxv_apply_spin_pair(from,to,create_up,create_dw,nterms,orb_up,orb_dw,coef,d_psi,d_out,norm2) bind(C,name="hxv_apply_spin_pair")
       import :: c_int, c_int32_t, c_ptr, c_double
       type(c_ptr),value             :: from,to,d_psi,d_out
       integer(c_int32_t),value      :: create_up,create_dw,nterms
       integer(c_int32_t),intent(in) :: orb_up(*),orb_dw(*)
       real(c_double),intent(in)     :: coef(*)
       real(c_double)                :: norm2
     end function hxv_apply_spin_pair
     integer(c_int) function hxv_apply_one_body(h,nterms,spin,orb_to,orb_from,coef,subtract_mean,d_psi,d_out,mean,norm2) bind(C,name="hxv_apply_one_body")
       import :: c_int, c_int32_t, c_ptr, c_double
       type(c_ptr),value             :: h,d_psi,d_out
       integer(c_int32_t),value      :: nterms,subtract_mean
       integer(c_int32_t),intent(in) :: spin(*),orb_to(*),orb_from(*)
       real(c_double),intent(in)     :: coef(*)
       real(c_double)                :: mean(2),norm2
     end function hxv_apply_one_body
     integer(c_int) function hxv_chebyshev_moments(h,d_vin,nprobes,d_probes,nmom,a,b,moments,self_moments) bind(C,name="hxv_chebyshev_moments")
       import :: c_int, c_int32_t, c_ptr, c_double, c_double_complex
       type(c_ptr),value         :: h,d_vin
       integer(c_int32_t),value  :: nprobes,nmom
       type(c_ptr)               :: d_probes(*)
       real(c_double),value      :: a,b
       complex(c_double_complex) :: moments(*)
       real(c_double)            :: self_moments(*)
     end function hxv_chebyshev_moments
     integer(c_int) function hxv_chebyshev_apply(h,d_vin,ncoef,coef,a,b,d_out,norm2) bind(C,name="hxv_chebyshev_apply")
       import :: c_int, c_int32_t, c_ptr, c_double, c_double_complex
       type(c_ptr),value                    :: h,d_vin,d_out
       integer(c_int32_t),value             :: ncoef
       complex(c_double_complex),intent(in) :: coef(*)
       real(c_double),value                 :: a,b
       real(c_double)                       :: norm2
     end function hxv_chebyshev_apply
     integer(c_int) function hxv_chebyshev_moments_real(h,d_vin,nprobes,d_probes,nmom,a,b,moments,self_moments) bind(C,name="hxv_chebyshev_moments_real")
       import :: c_int, c_int32_t, c_ptr, c_double
       type(c_ptr),value         :: h,d_vin
       integer(c_int32_t),value  :: nprobes,nmom
       type(c_ptr)               :: d_probes(*)
       real(c_double),value      :: a,b
       real(c_double)            :: moments(*)
       real(c_double)            :: self_moments(*)
     end function hxv_chebyshev_moments_real
     integer(c_int) function hxv_chebyshev_apply_real(h,d_vin,ncoef,coef,a,b,d_out,norm2) bind(C,name="hxv_chebyshev_apply_real")
       import :: c_int, c_int32_t, c_ptr, c_double
       type(c_ptr),value         :: h,d_vin,d_out
       integer(c_int32_t),value  :: ncoef
       real(c_double),intent(in) :: coef(*)
       real(c_double),value      :: a,b
       real(c_double)            :: norm2
     end function hxv_chebyshev_apply_real
     integer(c_int) function hxv_vector_random(h,seed,complex_valued,d_vec) bind(C,name="hxv_vector_random")
       import :: c_int, c_int32_t, c_int64_t, c_ptr
       type(c_ptr),value        :: h,d_vec
       integer(c_int64_t),value :: seed            !(uint64_t: the same 64 bits)
       integer(c_int32_t),value :: complex_valued
     end function hxv_vector_random
  end interface

  type(c_ptr),save :: handle = c_null_ptr   !one open sector at a time (ED_HAMILTONIAN_COMMON.f90:17-18)
  real(c_double),allocatable,save :: obs_record(:)   !the summed raw record of gpu_observables_dev (include/hxv.h)
  real(c_double),allocatable,save :: cdm_sum(:)      !the summed matrix of gpu_cluster_dm_dev, (re,im) pairs in cluster_density_matrix's order

contains

  subroutine check(ierr,where)
    integer(c_int)   :: ierr
    character(len=*) :: where
    character(kind=c_char),pointer :: msg(:)
    integer :: n
    if(ierr==0)return
    call c_f_pointer(hxv_last_error(),msg,[512])
    n=1
    do while(n<512.and.msg(n)/=c_null_char)
       n=n+1
    enddo
    write(*,"(A)")trim(where)//" ERROR: "//transfer(msg(1:n-1),repeat(" ",n-1))
    stop "hxv engine error"
  end subroutine check

  !> Device-side part of build_Hv_sector(isector): arguments are the module globals the reference
  !! has in scope at ED_HAMILTONIAN.f90:129 (Nlat..Nbath ED_INPUT_VARS.f90:13-16; impHloc
  !! ED_VARS_GLOBAL.f90:119; Hbath_reconstructed / diag_hybr as built at
  !! ED_HAMILTONIAN_SPARSE_HxV.f90:62-76; Uloc..xmu,hfmode ED_INPUT_VARS.f90:129-135,164;
  !! nup,ndw = get_Nup/get_Ndw(isector); MpiRank,MpiSize after the communicator shrink).
  subroutine gpu_build_Hv_sector(Nlat,Norb,Nspin,Nbath,nup,ndw,impHloc,Hbath,Vbath,Uloc,Ust,Jh,Jx,Jp,xmu,hfmode,MpiRank,MpiSize,device)
    integer,intent(in)                   :: Nlat,Norb,Nspin,Nbath,nup,ndw
    complex(8),intent(in),target,contiguous :: impHloc(:,:,:,:,:,:)   ![Nlat,Nlat,Nspin,Nspin,Norb,Norb]
    complex(8),intent(in),target,contiguous :: Hbath(:,:,:,:,:,:,:)   ![Nlat,Nlat,Nspin,Nspin,Norb,Norb,Nbath]
    real(8),intent(in),target,contiguous    :: Vbath(:,:,:,:)         ![Nlat,Nspin,Norb,Nbath]
    real(8),intent(in)                   :: Uloc(5),Ust,Jh,Jx,Jp,xmu
    logical,intent(in)                   :: hfmode
    integer,intent(in)                   :: MpiRank,MpiSize
    integer,intent(in),optional          :: device
    type(hxv_model)                      :: m
    integer                              :: dev
    if(c_associated(handle))stop "gpu_build_Hv_sector ERROR: a sector is already open"
    dev=0;if(present(device))dev=device
    m%nlat=Nlat; m%norb=Norb; m%nspin=Nspin; m%nbath=Nbath
    m%hfmode=0; if(hfmode)m%hfmode=1
    m%reserved=0
    m%uloc=Uloc
    m%ust=Ust; m%jh=Jh; m%jx=Jx; m%jp=Jp; m%xmu=xmu
    m%imphloc=c_loc(impHloc)
    m%hbath=c_null_ptr; m%vbath=c_null_ptr
    if(Nbath>0)then
       m%hbath=c_loc(Hbath)
       m%vbath=c_loc(Vbath)
    endif
    call check(hxv_create_from_model(m,int(nup,c_int32_t),int(ndw,c_int32_t),int(MpiRank,c_int32_t),&
         int(MpiSize,c_int32_t),int(dev,c_int32_t),handle),"gpu_build_Hv_sector")
    call sector_opened()
    call check(hxv_set_option(handle,"eigh_degenerate"//c_null_char,merge(1_c_int64_t,0_c_int64_t,gpu_eigh_degenerate)),"gpu_build_Hv_sector")
  end subroutine gpu_build_Hv_sector

  !---- reference tables of the device vectors (see type ref_entry) ----
  integer function ref_find(tab,id) result(i)
    type(ref_entry),intent(in) :: tab(:)
    integer(8),intent(in)      :: id
    if(id/=0)then
       do i=1,size(tab)
          if(tab(i)%n>0.and.tab(i)%id==id)return
       enddo
    endif
    i=0
  end function ref_find
  subroutine ref_add(tab,id)
    type(ref_entry),intent(inout) :: tab(:)
    integer(8),intent(in)         :: id
    integer                       :: i
    i=ref_find(tab,id)
    if(i==0)then
       do i=1,size(tab)
          if(tab(i)%n==0)exit
       enddo
       if(i>size(tab))stop "ED_HAMILTONIAN_GPU_HxV ERROR: more than 512 live device vectors / sectors"
       tab(i)%id=id; tab(i)%kept=.false.; tab(i)%dead=.false.
    endif
    tab(i)%n=tab(i)%n+1
  end subroutine ref_add
  !a new gpu_vector of the OPEN sector, in allocation `base`: its own (view=.false.: a fresh serial) or the one `owner` lives in
  subroutine vec_born(vect,base,view,owner)
    type(gpu_vector),intent(inout)       :: vect
    type(c_ptr),intent(in)               :: base
    logical,intent(in)                   :: view
    type(gpu_vector),intent(in),optional :: owner
    vect%sector=handle; vect%sector_id=handle_serial; vect%base=base; vect%view=view; vect%owns_sector=.false.
    if(view)then
       if(.not.present(owner))stop "ED_HAMILTONIAN_GPU_HxV ERROR: a view needs the vector that owns its allocation"
       vect%alloc_id=owner%alloc_id
    else
       next_serial=next_serial+1
       vect%alloc_id=next_serial
    endif
    call ref_add(alloc_refs,vect%alloc_id)
    call ref_add(sector_refs,vect%sector_id)
  end subroutine vec_born
  !a device vector that can still be used: made, not freed, its sector not closed under it
  logical function vec_alive(vect) result(ok)
    type(gpu_vector),intent(in) :: vect
    integer                     :: i
    ok=.false.
    if(.not.c_associated(vect%d))return
    i=ref_find(sector_refs,vect%sector_id)
    if(i==0)return
    ok=.not.sector_refs(i)%dead
  end function vec_alive
  !the open sector got its serial (every build_Hv_sector variant calls this right after the engine returned the handle)
  subroutine sector_opened()
    next_serial=next_serial+1
    handle_serial=next_serial
  end subroutine sector_opened

  !> delete_Hv_sector hook (ED_HAMILTONIAN.f90:149-190)
  subroutine gpu_delete_Hv_sector()
    integer :: i
    if(c_associated(handle))then
       i=ref_find(sector_refs,handle_serial)
       if(i>0)sector_refs(i)%dead=.true.   !vectors of this sector are still alive: hxv_destroy takes their memory back, their shells stay
       call check(hxv_destroy(handle),"gpu_delete_Hv_sector")
    endif
    handle=c_null_ptr; handle_serial=0
  end subroutine gpu_delete_Hv_sector

  !> vecDim_Hv_sector of the open sector (ED_HAMILTONIAN.f90:197-221)
  function gpu_vecDim_Hv_sector() result(vecDim)
    integer :: vecDim
    if(.not.c_associated(handle))stop "gpu_vecDim_Hv_sector ERROR: Hsector NOT set"
    vecDim=int(hxv_vecdim(handle))
  end function gpu_vecDim_Hv_sector

  !> The product, with the cc_sparse_HxV interface (ED_VARS_GLOBAL.f90:72-78): Hv = H*v.
  subroutine gpuMatVec_main(Nloc,v,Hv)
    integer                    :: Nloc
    complex(8),dimension(Nloc) :: v
    complex(8),dimension(Nloc) :: Hv
    if(.not.c_associated(handle))stop "gpuMatVec_main ERROR: Hsector NOT set"
    call check(hxv_apply_host(handle,int(Nloc,c_int64_t),v,Hv),"gpuMatVec_main")
  end subroutine gpuMatVec_main

  !> Target of the pointer when MpiStatus=T (the reference binds spMatVec_MPI_main there, ED_HAMILTONIAN.f90:131-134):
  !! v, Hv are this rank's slab of vecDim_Hv_sector elements; the engine all-gathers the slabs itself (hxv_apply_host).
  subroutine gpuMatVec_MPI_main(Nloc,v,Hv)
    integer                    :: Nloc
    complex(8),dimension(Nloc) :: v
    complex(8),dimension(Nloc) :: Hv
    if(.not.c_associated(handle))stop "gpuMatVec_MPI_main ERROR: Hsector NOT set"
    call check(hxv_apply_host(handle,int(Nloc,c_int64_t),v,Hv),"gpuMatVec_MPI_main")
  end subroutine gpuMatVec_MPI_main

  !> Communicator of the open (split) sector.  Host side, after gpu_build_Hv_sector on every rank of MpiComm:
  !!     if(MpiRank==0)call gpu_comm_unique_id(id)
  !!     call MPI_Bcast(id,128,MPI_BYTE,0,MpiComm,ierr)
  !!     call gpu_comm_init(id)
  !! (gpu_delete_Hv_sector releases it with the sector.)
  subroutine gpu_comm_unique_id(id)
    integer(c_int8_t),intent(out) :: id(128)
    call check(hxv_comm_unique_id(id),"gpu_comm_unique_id")
  end subroutine gpu_comm_unique_id

  subroutine gpu_comm_init(id)
    integer(c_int8_t),intent(in) :: id(128)
    if(.not.c_associated(handle))stop "gpu_comm_init ERROR: Hsector NOT set"
    call check(hxv_comm_init(handle,id),"gpu_comm_init")
  end subroutine gpu_comm_init

  !> Plain Lanczos tridiagonalisation driven through a cc_sparse_HxV procedure on HOST vectors:
  !! the call shape of SciFortran's sp_lanc_tridiag(MatVec,vin,alanc,blanc) as consumed at
  !! ED_GF_NORMAL.f90:215-220,949-951 (alanc(k)=<q_k|H|q_k>, blanc(k+1)=beta_{k+1}, blanc(1) unused).
  !! SciFortran is not vendored with the reference; this stands where it would be linked.
  subroutine gpu_lanc_tridiag_host(MatVec,vin,alanc,blanc,threshold)
    interface
       subroutine MatVec(Nloc,v,Hv)
         integer                    :: Nloc
         complex(8),dimension(Nloc) :: v,Hv
       end subroutine MatVec
    end interface
    complex(8),intent(inout) :: vin(:)
    real(8),intent(inout)    :: alanc(:),blanc(:)
    real(8),intent(in),optional :: threshold
    complex(8),allocatable   :: q(:),qm(:),w(:)
    real(8)                  :: a,b,thr
    integer                  :: k,n,nlanc
    n=size(vin); nlanc=size(alanc)
    thr=1d-12; if(present(threshold))thr=threshold
    allocate(q(n),qm(n),w(n))
    q=vin/sqrt(dble(dot_product(vin,vin))); qm=(0d0,0d0); b=0d0
    alanc=0d0; blanc=0d0
    do k=1,nlanc
       call MatVec(n,q,w)
       w=w-b*qm
       a=dble(dot_product(q,w))
       w=w-a*q
       alanc(k)=a
       b=sqrt(dble(dot_product(w,w)))
       if(k<nlanc)blanc(k+1)=b
       if(abs(b)<thr)exit
       qm=q
       q=w/b
    enddo
    deallocate(q,qm,w)
  end subroutine gpu_lanc_tridiag_host

  !> Device-resident Lanczos with the SciFortran CALL SIGNATURES, so that the two call sites can switch by
  !! changing one `use`:   sp_lanc_tridiag(MatVec,vin,alanc,blanc)        ED_GF_NORMAL.f90:215-220 (+7)
  !!                        sp_lanc_eigh(MatVec,egs,vect,Nitermax,iverbose,threshold)   ED_DIAG.f90:176-184
  !! MatVec is accepted for signature compatibility and not called: the product of the OPEN sector runs on the
  !! device; vin/vect cross PCIe once per run instead of twice per iteration.
  subroutine gpu_sp_lanc_tridiag_serial(MatVec,vin,alanc,blanc,threshold)
    interface
       subroutine MatVec(Nloc,v,Hv)
         integer                    :: Nloc
         complex(8),dimension(Nloc) :: v,Hv
       end subroutine MatVec
    end interface
    complex(8),intent(inout)    :: vin(:)
    real(8),intent(inout)       :: alanc(:),blanc(:)
    real(8),intent(in),optional :: threshold
    real(8)                     :: thr
    integer(c_int32_t)          :: nsteps
    if(.not.c_associated(handle))stop "gpu_sp_lanc_tridiag ERROR: Hsector NOT set"
    thr=1d-12; if(present(threshold))thr=threshold
    !(the engine normalises the start vector itself, as SciFortran's sp_lanc_tridiag does on its first iteration; on a
    ! split sector the norm is the global one)
    call check(hxv_lanczos_tridiag_host(handle,vin,int(size(alanc),c_int32_t),alanc,blanc,thr,nsteps),"gpu_sp_lanc_tridiag")
  end subroutine gpu_sp_lanc_tridiag_serial

  !> TWO tridiagonalisations on one product (real H): two of the independent channels of lanc_build_gf_normal_*
  !! (ED_GF_NORMAL.f90:123-306; one sp_lanc_tridiag each at :215,282,422,504,638,720,801,882) share the product's passes, their
  !! real start vectors travelling as real and imaginary part of one complex Lanczos vector (H(x+iy) = Hx + iHy).  Same
  !! argument meaning as sp_lanc_tridiag, once per channel; vin_a, vin_b must have zero imaginary parts.
  subroutine gpu_sp_lanc_tridiag_pair(MatVec,vin_a,vin_b,alanc_a,blanc_a,alanc_b,blanc_b,threshold)
    interface
       subroutine MatVec(Nloc,v,Hv)
         integer                    :: Nloc
         complex(8),dimension(Nloc) :: v,Hv
       end subroutine MatVec
    end interface
    complex(8),intent(inout)    :: vin_a(:),vin_b(:)
    real(8),intent(inout)       :: alanc_a(:),blanc_a(:),alanc_b(:),blanc_b(:)
    real(8),intent(in),optional :: threshold
    real(8)                     :: thr
    integer(c_int32_t)          :: na,nb
    if(.not.c_associated(handle))stop "gpu_sp_lanc_tridiag_pair ERROR: Hsector NOT set"
    if(size(alanc_a)/=size(alanc_b))stop "gpu_sp_lanc_tridiag_pair ERROR: the two channels need equally long alanc/blanc"
    thr=1d-12; if(present(threshold))thr=threshold
    call check(hxv_lanczos_tridiag_pair_host(handle,vin_a,vin_b,int(size(alanc_a),c_int32_t),alanc_a,blanc_a,alanc_b,blanc_b,thr,na,nb),&
         "gpu_sp_lanc_tridiag_pair")
  end subroutine gpu_sp_lanc_tridiag_pair

  subroutine gpu_sp_lanc_eigh_serial(MatVec,egs,vect,Nitermax,iverbose,threshold)
    interface
       subroutine MatVec(Nloc,v,Hv)
         integer                    :: Nloc
         complex(8),dimension(Nloc) :: v,Hv
       end subroutine MatVec
    end interface
    real(8),intent(inout)       :: egs
    complex(8),intent(inout)    :: vect(:)
    integer,intent(in)          :: Nitermax
    logical,intent(in),optional :: iverbose
    real(8),intent(in),optional :: threshold
    real(8)                     :: thr
    integer(c_int32_t)          :: niter
    if(.not.c_associated(handle))stop "gpu_sp_lanc_eigh ERROR: Hsector NOT set"
    thr=1d-12; if(present(threshold))thr=max(threshold,1d-15)
    call check(hxv_lanczos_eigh_host(handle,int(Nitermax,c_int32_t),thr,egs,vect,niter),"gpu_sp_lanc_eigh")
    if(present(iverbose))then
       if(iverbose)write(*,"(A,I6,A,F20.12)")"gpu_sp_lanc_eigh: iterations=",niter," E0=",egs
    endif
  end subroutine gpu_sp_lanc_eigh_serial

  !> sp_eigh(MatVec,eval,evec,Nblock,Nitermax,tol,iverbose) -- the default (lanc_method="arpack") spectrum call at
  !! ED_DIAG.f90:152-160 -- on the device: size(eval) lowest eigenpairs, Krylov basis of Nblock vectors in HBM.
  subroutine gpu_sp_eigh_serial(MatVec,eval,evec,Nblock,Nitermax,tol,iverbose)
    interface
       subroutine MatVec(Nloc,v,Hv)
         integer                    :: Nloc
         complex(8),dimension(Nloc) :: v,Hv
       end subroutine MatVec
    end interface
    real(8),intent(inout)       :: eval(:)
    complex(8),intent(inout)    :: evec(:,:)
    integer,intent(in),optional :: Nblock,Nitermax
    real(8),intent(in),optional :: tol
    logical,intent(in),optional :: iverbose
    integer(c_int32_t)          :: ncv,nit,nconv,nmv
    real(8)                     :: tl
    if(.not.c_associated(handle))stop "gpu_sp_eigh ERROR: Hsector NOT set"
    if(size(evec,2)<size(eval))stop "gpu_sp_eigh ERROR: size(evec,2) < size(eval)"
    ncv=0;   if(present(Nblock))ncv=int(Nblock,c_int32_t)
    !Nblock = min(dim,lanc_ncv_factor*max(Neigen,lanc_nstates_sector)+lanc_ncv_add) (ED_DIAG.f90:96) exceeds the engine's
    !largest Krylov basis (64 vectors) once lanc_nstates_sector >= 7: clamp instead of stopping the run
    if(ncv>64)then
       write(*,"(A,I6,A)")"gpu_sp_eigh WARNING: Nblock=",ncv," > 64: using a Krylov basis of 64 vectors"
       ncv=64
    endif
    if(size(eval)>=64)stop "gpu_sp_eigh ERROR: more than 63 eigenpairs per sector exceed the engine's Krylov basis (64 vectors)"
    !Nitermax bounds the RESTARTS here (each restart is up to ncv products; ARPACK's bound counts restarts too)
    nit=512; if(present(Nitermax))nit=int(Nitermax,c_int32_t)
    tl=0d0;  if(present(tol))tl=tol
    call check(hxv_eigh_lowest_host(handle,int(size(eval),c_int32_t),ncv,nit,tl,eval,evec,nconv,nmv),"gpu_sp_eigh")
    if(present(iverbose))then
       if(iverbose)write(*,"(A,I4,A,I6,A,F20.12)")"gpu_sp_eigh: converged=",nconv," matvecs=",nmv," E0=",eval(1)
    endif
  end subroutine gpu_sp_eigh_serial

  !> ---------------------------------------------------------------------------------------------------------------------------
  !! DEVICE-RESIDENT Green's-function channel.  The reference builds every channel on the host (ED_GF_NORMAL.f90:174-217): the ground
  !! state comes out of the eigensolver into a host array, c^dagger|gs> is formed by a serial loop on the master, scattered, and handed
  !! to sp_lanc_tridiag -- with the drivers above that is three Dim-sized PCIe transfers per channel.  Here the ground state stays where
  !! the eigensolver left it and the start vector is made next to it:
  !!     call gpu_build_Hv_sector(...isector...)                        !sector of the ground state
  !!     call gpu_sp_lanc_eigh_dev(egs,gs,Nitermax,threshold)           !gs: type(gpu_vector), stays on the device
  !!     call gpu_keep_sector(gs)                                       !the sector stays open for gs; another one can be built
  !!     call gpu_build_Hv_sector(...jsector...)                        !sector of c^dagger|gs>  (ED_GF_NORMAL.f90:176)
  !!     call gpu_apply_ladder(gs,ipos,ispin,.true.,vv,norm2)           !vv = c^dagger_{ipos,ispin}|gs>, norm2 = <vv|vv>  (:180-199)
  !!     call gpu_sp_lanc_tridiag_dev(vv,alfa_,beta_)                   !(:215) the engine normalises vv itself
  !!     call gpu_free_vector(vv); call gpu_delete_Hv_sector()
  !!     ... further channels from the same gs ...
  !!     call gpu_free_vector(gs)                                       !closes the ground state's sector too
  !! Mixed channels (:370-406, :746-780): a second gpu_apply_ladder into the same vv with accumulate=.true. and coef.
  !! On a split sector (after gpu_comm_init) every rank holds and builds its own slab.
  !! ---------------------------------------------------------------------------------------------------------------------------
  subroutine gpu_sp_lanc_eigh_dev(egs,vect,Nitermax,iverbose,threshold)
    real(8),intent(inout)          :: egs
    type(gpu_vector),intent(inout) :: vect
    integer,intent(in)             :: Nitermax
    logical,intent(in),optional    :: iverbose
    real(8),intent(in),optional    :: threshold
    real(8)                        :: thr
    integer(c_int32_t)             :: niter
    if(.not.c_associated(handle))stop "gpu_sp_lanc_eigh_dev ERROR: Hsector NOT set"
    if(c_associated(vect%d))stop "gpu_sp_lanc_eigh_dev ERROR: the vector is in use (gpu_free_vector it first)"
    call check(hxv_vector_alloc(handle,vect%d),"gpu_sp_lanc_eigh_dev")
    call vec_born(vect,vect%d,.false.)
    thr=1d-12; if(present(threshold))thr=max(threshold,1d-15)
    call check(hxv_lanczos_eigh(handle,int(Nitermax,c_int32_t),thr,egs,vect%d,niter),"gpu_sp_lanc_eigh_dev")
    if(present(iverbose))then
       if(iverbose)write(*,"(A,I6,A,F20.12)")"gpu_sp_lanc_eigh_dev: iterations=",niter," E0=",egs
    endif
  end subroutine gpu_sp_lanc_eigh_dev

  !> sp_eigh (the default lanc_method="arpack" call, ED_DIAG.f90:152-160) with the eigenvectors left on the device: vects(1:size(eval)), all in
  !! one allocation that is returned to the engine when the LAST of them is freed (any order).  Any of them can be handed to
  !! gpu_keep_sector / gpu_apply_ladder like the vector of gpu_sp_lanc_eigh_dev.
  subroutine gpu_sp_eigh_dev(eval,vects,Nblock,Nitermax,tol,iverbose)
    real(8),intent(inout)          :: eval(:)
    type(gpu_vector),intent(inout) :: vects(:)
    integer,intent(in),optional    :: Nblock,Nitermax
    real(8),intent(in),optional    :: tol
    logical,intent(in),optional    :: iverbose
    integer(c_int32_t)             :: ncv,nit,nconv,nmv
    real(8)                        :: tl
    integer                        :: i
    integer(c_int64_t)             :: stride
    complex(c_double_complex),pointer :: base(:)
    if(.not.c_associated(handle))stop "gpu_sp_eigh_dev ERROR: Hsector NOT set"
    if(size(vects)<size(eval))stop "gpu_sp_eigh_dev ERROR: size(vects) < size(eval)"
    if(size(eval)>=64)stop "gpu_sp_eigh_dev ERROR: more than 63 eigenpairs per sector exceed the engine's Krylov basis (64 vectors)"
    do i=1,size(eval)
       if(c_associated(vects(i)%d))stop "gpu_sp_eigh_dev ERROR: a vector is in use (gpu_free_vector it first)"
    enddo
    ncv=0;   if(present(Nblock))ncv=int(min(Nblock,64),c_int32_t)
    nit=512; if(present(Nitermax))nit=int(Nitermax,c_int32_t)
    tl=0d0;  if(present(tol))tl=tol
    call check(hxv_vector_alloc_many(handle,int(size(eval),c_int32_t),vects(1)%d),"gpu_sp_eigh_dev")
    stride=hxv_localvec_elems(handle)
    call c_f_pointer(vects(1)%d,base,[stride*size(eval)])      !(address arithmetic only: the memory is on the device)
    do i=1,size(eval)
       if(i>1)vects(i)%d=c_loc(base(1+(i-1)*stride))
       if(i==1)then; call vec_born(vects(1),vects(1)%d,.false.); else; call vec_born(vects(i),vects(1)%d,.true.,vects(1)); endif
    enddo
    call check(hxv_eigh_lowest(handle,int(size(eval),c_int32_t),ncv,nit,tl,eval,vects(1)%d,nconv,nmv),"gpu_sp_eigh_dev")
    if(present(iverbose))then
       if(iverbose)write(*,"(A,I4,A,I6,A,F20.12)")"gpu_sp_eigh_dev: converged=",nconv," matvecs=",nmv," E0=",eval(1)
    endif
  end subroutine gpu_sp_eigh_dev

  !> The open sector stays open for the vectors made on it (it is needed again when c / c^dagger act on them); the module's "one open
  !! sector" slot becomes free, so build_Hv_sector of another sector may follow.  The kept sector is closed when the LAST vector made on
  !! it is freed (gpu_free_vector), in whatever order -- eigenvectors 2.. of gpu_sp_eigh_dev included.
  subroutine gpu_keep_sector(vect)
    type(gpu_vector),intent(inout) :: vect
    integer                        :: i
    if(.not.c_associated(handle))stop "gpu_keep_sector ERROR: Hsector NOT set"
    if(vect%sector_id/=handle_serial.or..not.c_associated(vect%d))stop "gpu_keep_sector ERROR: the vector does not belong to the open sector"
    i=ref_find(sector_refs,handle_serial)
    if(i==0)stop "gpu_keep_sector ERROR: no live vector of the open sector"
    sector_refs(i)%kept=.true.
    vect%owns_sector=.true.
    handle=c_null_ptr; handle_serial=0
  end subroutine gpu_keep_sector

  !> out = [out +] coef * c^(dagger)_{ipos,ispin} psi, from psi's sector into the OPEN sector; norm2 = <out|out> afterwards.
  !! ipos = 1-based orbital position in the spin string (iorb+(ilat-1)*Norb, ED_GF_NORMAL.f90:176-199), ispin = 1 (up) | 2 (dw).
  subroutine gpu_apply_ladder(psi,ipos,ispin,create,out,norm2,coef,accumulate)
    type(gpu_vector),intent(in)    :: psi
    integer,intent(in)             :: ipos,ispin
    logical,intent(in)             :: create
    type(gpu_vector),intent(inout) :: out
    real(8),intent(out)            :: norm2
    complex(8),intent(in),optional :: coef
    logical,intent(in),optional    :: accumulate
    complex(8)                     :: cf
    integer(c_int32_t)             :: acc,cr
    if(.not.c_associated(handle))stop "gpu_apply_ladder ERROR: Hsector NOT set (build the target sector first)"
    if(.not.vec_alive(psi))stop "gpu_apply_ladder ERROR: empty source vector, or its sector was closed under it (gpu_keep_sector keeps it open)"
    cf=(1d0,0d0); if(present(coef))cf=coef
    acc=0; if(present(accumulate))then; if(accumulate)acc=1; endif
    if(.not.c_associated(out%d))then
       if(acc==1)stop "gpu_apply_ladder ERROR: accumulate into an empty vector"
       call check(hxv_vector_alloc(handle,out%d),"gpu_apply_ladder")
       call vec_born(out,out%d,.false.)
    endif
    if(out%sector_id/=handle_serial)stop "gpu_apply_ladder ERROR: the target vector does not belong to the open sector"
    cr=0; if(create)cr=1
    call check(hxv_apply_ladder_axpy(psi%sector,handle,int(ipos-1,c_int32_t),int(ispin-1,c_int32_t),cr,dble(cf),aimag(cf),acc,psi%d,out%d,norm2),&
         "gpu_apply_ladder")
  end subroutine gpu_apply_ladder

  !> out = psi as a vector of its twin sector: from psi's sector (nup,ndw) into the OPEN sector, which must be (ndw,nup).  The twin branch of
  !! es_return_cvector (ED_EIGENSPACE.f90:485-494, vector(i)=twin%cvec(Order(i)), Order of ED_SETUP.f90:854-898) on the device: with ed_twin
  !! the state found in one sector of a pair serves the other one without a Dim-sized PCIe transfer.  No sign; an eigenstate of the open
  !! sector for spin-symmetric models only (the reference warns for Nspin>1).  On split sectors (psi's sector and the open one the same rank
  !! of the same MpiSize, the open one bound to the communicator) psi and out are this rank's slabs and the call is collective: one
  !! all-to-all between two kernels instead of es_return_cvector_mpi's gather on the master (ED_EIGENSPACE.f90:498-569).
  subroutine gpu_twin_vector(psi,out)
    type(gpu_vector),intent(in)    :: psi
    type(gpu_vector),intent(inout) :: out
    if(.not.c_associated(handle))stop "gpu_twin_vector ERROR: Hsector NOT set (build the target sector first)"
    if(.not.vec_alive(psi))stop "gpu_twin_vector ERROR: empty source vector, or its sector was closed under it (gpu_keep_sector keeps it open)"
    if(.not.c_associated(out%d))then
       call check(hxv_vector_alloc(handle,out%d),"gpu_twin_vector")
       call vec_born(out,out%d,.false.)
    endif
    if(out%sector_id/=handle_serial)stop "gpu_twin_vector ERROR: the target vector does not belong to the open sector"
    call check(hxv_twin_vector(psi%sector,handle,psi%d,out%d),"gpu_twin_vector")
  end subroutine gpu_twin_vector

  !> sp_lanc_tridiag (ED_GF_NORMAL.f90:215) from a start vector that is on the device already (normalised by the engine).
  subroutine gpu_sp_lanc_tridiag_dev(vin,alanc,blanc,threshold)
    type(gpu_vector),intent(in) :: vin
    real(8),intent(inout)       :: alanc(:),blanc(:)
    real(8),intent(in),optional :: threshold
    real(8)                     :: thr
    integer(c_int32_t)          :: nsteps
    if(.not.c_associated(handle))stop "gpu_sp_lanc_tridiag_dev ERROR: Hsector NOT set"
    if(vin%sector_id/=handle_serial.or..not.c_associated(vin%d))stop "gpu_sp_lanc_tridiag_dev ERROR: the start vector does not belong to the open sector"
    thr=1d-12; if(present(threshold))thr=threshold
    call check(hxv_lanczos_tridiag(handle,vin%d,int(size(alanc),c_int32_t),alanc,blanc,thr,nsteps),"gpu_sp_lanc_tridiag_dev")
  end subroutine gpu_sp_lanc_tridiag_dev

  !> TWO channels of the same sector on one product (real H; gpu_sp_lanc_tridiag_pair with start vectors that are on the device already):
  !! e.g. c^dagger_{i,up}|gs> and c^dagger_{j,up}|gs> of one ground state -- both real, both in the open sector.
  subroutine gpu_sp_lanc_tridiag_pair_dev(vin_a,vin_b,alanc_a,blanc_a,alanc_b,blanc_b,threshold)
    type(gpu_vector),intent(in) :: vin_a,vin_b
    real(8),intent(inout)       :: alanc_a(:),blanc_a(:),alanc_b(:),blanc_b(:)
    real(8),intent(in),optional :: threshold
    real(8)                     :: thr
    integer(c_int32_t)          :: na,nb
    if(.not.c_associated(handle))stop "gpu_sp_lanc_tridiag_pair_dev ERROR: Hsector NOT set"
    if(vin_a%sector_id/=handle_serial.or.vin_b%sector_id/=handle_serial.or..not.c_associated(vin_a%d).or..not.c_associated(vin_b%d))&
         stop "gpu_sp_lanc_tridiag_pair_dev ERROR: the start vectors do not belong to the open sector"
    if(size(alanc_a)/=size(alanc_b))stop "gpu_sp_lanc_tridiag_pair_dev ERROR: the two channels need equally long alanc/blanc"
    thr=1d-12; if(present(threshold))thr=threshold
    call check(hxv_lanczos_tridiag_pair(handle,vin_a%d,vin_b%d,int(size(alanc_a),c_int32_t),alanc_a,blanc_a,alanc_b,blanc_b,thr,na,nb),&
         "gpu_sp_lanc_tridiag_pair_dev")
  end subroutine gpu_sp_lanc_tridiag_pair_dev

  !> gpu_sp_lanc_tridiag_dev with PROBE vectors (include/hxv.h, hxv_lanczos_tridiag_probes): besides alanc / blanc the overlaps
  !! overlaps(j,k) = <probes(j)|q_k> of every unit Lanczos vector q_k, k = 1..nsteps, with up to 8 device vectors of the open sector (e.g.
  !! c^dagger_j|gs> for the other orbitals j while the run starts from c^dagger_i|gs>): what gpu_gf_from_probes turns into the off-diagonal
  !! Green's functions of orbital i, so that ONE run per orbital replaces lanc_build_gf_normal_mix_chan2/4 (ED_GF_NORMAL.f90:315-903).
  !! overlaps is (size(probes), size(alanc)); columns of steps that did not run are zero; nsteps = the steps done.
  subroutine gpu_sp_lanc_tridiag_probes_dev(vin,probes,alanc,blanc,overlaps,threshold,nsteps)
    type(gpu_vector),intent(in)  :: vin
    type(gpu_vector),intent(in)  :: probes(:)
    real(8),intent(inout)        :: alanc(:),blanc(:)
    complex(8),intent(inout)     :: overlaps(:,:)
    real(8),intent(in),optional  :: threshold
    integer,intent(out),optional :: nsteps
    real(8)                      :: thr
    integer(c_int32_t)           :: ns
    type(c_ptr)                  :: plist(8)
    complex(8),allocatable       :: ov(:,:)
    integer                      :: j
    if(.not.c_associated(handle))stop "gpu_sp_lanc_tridiag_probes_dev ERROR: Hsector NOT set"
    if(vin%sector_id/=handle_serial.or..not.c_associated(vin%d))stop "gpu_sp_lanc_tridiag_probes_dev ERROR: the start vector does not belong to the open sector"
    if(size(probes)>8)stop "gpu_sp_lanc_tridiag_probes_dev ERROR: more than 8 probes"
    if(size(overlaps,1)/=size(probes).or.size(overlaps,2)/=size(alanc).or.size(blanc)/=size(alanc))&
         stop "gpu_sp_lanc_tridiag_probes_dev ERROR: overlaps must be (size(probes),size(alanc)), blanc as long as alanc"
    plist=c_null_ptr
    do j=1,size(probes)
       if(probes(j)%sector_id/=handle_serial.or..not.c_associated(probes(j)%d))stop "gpu_sp_lanc_tridiag_probes_dev ERROR: a probe does not belong to the open sector"
       plist(j)=probes(j)%d
    enddo
    thr=1d-12; if(present(threshold))thr=threshold
    allocate(ov(max(size(probes),1),size(alanc)))      !(contiguous, whatever section the caller passed)
    call check(hxv_lanczos_tridiag_probes(handle,vin%d,int(size(probes),c_int32_t),plist,int(size(alanc),c_int32_t),alanc,blanc,ov,thr,ns),&
         "gpu_sp_lanc_tridiag_probes_dev")
    if(size(probes)>0)overlaps=ov
    if(present(nsteps))nsteps=int(ns)
  end subroutine gpu_sp_lanc_tridiag_probes_dev

  !> Chebyshev moments of a device vector of the open sector (include/hxv.h, hxv_chebyshev_moments): with Ht = (H - b)/a and the spectrum
  !! of H inside [b-a, b+a],
  !!     moments(j,n) = <probes(j)|T_{n-1}(Ht)|vin>,  n = 1..size(moments,2),  from size(moments,2)-1 products,
  !!     self_moments(k) = <vin|T_{k-1}(Ht)|vin>,  k = 1..2*size(moments,2)-1  (optional), from the same products.
  !! vin is used as given (not normalised) and only read; up to 8 probes, none is allowed (moments is then (0,nmom) and only its second
  !! extent is used).  A window that does not hold the spectrum stops the program with the engine's message ("spectrum outside the window").
  subroutine gpu_chebyshev_moments_dev(vin,probes,a,b,moments,self_moments)
    type(gpu_vector),intent(in)      :: vin
    type(gpu_vector),intent(in)      :: probes(:)
    real(8),intent(in)               :: a,b
    complex(8),intent(inout)         :: moments(:,:)
    real(8),intent(inout),optional   :: self_moments(:)
    type(c_ptr)                      :: plist(8)
    complex(8),allocatable           :: mom(:,:)
    real(8),allocatable              :: smom(:)
    integer                          :: j,nmom
    if(.not.c_associated(handle))stop "gpu_chebyshev_moments_dev ERROR: Hsector NOT set"
    if(vin%sector_id/=handle_serial.or..not.c_associated(vin%d))stop "gpu_chebyshev_moments_dev ERROR: the start vector does not belong to the open sector"
    if(size(probes)>8)stop "gpu_chebyshev_moments_dev ERROR: more than 8 probes"
    nmom=size(moments,2)
    if(size(moments,1)/=size(probes).or.nmom<1)stop "gpu_chebyshev_moments_dev ERROR: moments must be (size(probes),nmom), nmom >= 1"
    if(present(self_moments))then
       if(size(self_moments)/=2*nmom-1)stop "gpu_chebyshev_moments_dev ERROR: self_moments must have 2*nmom-1 entries"
    endif
    plist=c_null_ptr
    do j=1,size(probes)
       if(probes(j)%sector_id/=handle_serial.or..not.c_associated(probes(j)%d))stop "gpu_chebyshev_moments_dev ERROR: a probe does not belong to the open sector"
       plist(j)=probes(j)%d
    enddo
    allocate(mom(max(size(probes),1),nmom),smom(2*nmom-1))      !(contiguous, whatever section the caller passed)
    call check(hxv_chebyshev_moments(handle,vin%d,int(size(probes),c_int32_t),plist,int(nmom,c_int32_t),a,b,mom,smom),"gpu_chebyshev_moments_dev")
    if(size(probes)>0)moments=mom
    if(present(self_moments))self_moments=smom
  end subroutine gpu_chebyshev_moments_dev

  !> A polynomial of H on a device vector of the open sector (include/hxv.h, hxv_chebyshev_apply):
  !!     out = sum_{n=1}^{size(coef)} coef(n) T_{n-1}(Ht) vin,   norm2 = <out|out>,
  !! size(coef)-1 products; coef from the series of e^{-tau H} or e^{-iHt} on the window (a,b).  vin is only read; an empty out is
  !! allocated on the open sector; out must not be vin.
  subroutine gpu_chebyshev_apply_dev(vin,coef,a,b,out,norm2)
    type(gpu_vector),intent(in)    :: vin
    complex(8),intent(in)          :: coef(:)
    real(8),intent(in)             :: a,b
    type(gpu_vector),intent(inout) :: out
    real(8),intent(out),optional   :: norm2
    complex(8),allocatable         :: cf(:)
    real(8)                        :: n2
    if(.not.c_associated(handle))stop "gpu_chebyshev_apply_dev ERROR: Hsector NOT set"
    if(vin%sector_id/=handle_serial.or..not.c_associated(vin%d))stop "gpu_chebyshev_apply_dev ERROR: the start vector does not belong to the open sector"
    if(size(coef)<1)stop "gpu_chebyshev_apply_dev ERROR: at least one coefficient"
    if(.not.c_associated(out%d))then
       call check(hxv_vector_alloc(handle,out%d),"gpu_chebyshev_apply_dev")
       call vec_born(out,out%d,.false.)
    endif
    if(out%sector_id/=handle_serial)stop "gpu_chebyshev_apply_dev ERROR: the output does not belong to the open sector"
    allocate(cf(size(coef))); cf=coef                           !(contiguous, whatever section the caller passed)
    n2=0d0
    call check(hxv_chebyshev_apply(handle,vin%d,int(size(coef),c_int32_t),cf,a,b,out%d,n2),"gpu_chebyshev_apply_dev")
    if(present(norm2))norm2=n2
  end subroutine gpu_chebyshev_apply_dev

  !> gpu_chebyshev_moments_dev on REAL vectors (include/hxv.h, hxv_chebyshev_moments_real): a real H, vin and the probes purely real (device
  !! vectors of the open sector in their ordinary layout); moments are REAL.  Half the bytes per order.  An imaginary part in a vector, or a
  !! sector without real vectors, stops the program with the engine's message.
  subroutine gpu_chebyshev_moments_real_dev(vin,probes,a,b,moments,self_moments)
    type(gpu_vector),intent(in)      :: vin
    type(gpu_vector),intent(in)      :: probes(:)
    real(8),intent(in)               :: a,b
    real(8),intent(inout)            :: moments(:,:)
    real(8),intent(inout),optional   :: self_moments(:)
    type(c_ptr)                      :: plist(8)
    real(8),allocatable              :: mom(:,:),smom(:)
    integer                          :: j,nmom
    if(.not.c_associated(handle))stop "gpu_chebyshev_moments_real_dev ERROR: Hsector NOT set"
    if(vin%sector_id/=handle_serial.or..not.c_associated(vin%d))stop "gpu_chebyshev_moments_real_dev ERROR: the start vector does not belong to the open sector"
    if(size(probes)>8)stop "gpu_chebyshev_moments_real_dev ERROR: more than 8 probes"
    nmom=size(moments,2)
    if(size(moments,1)/=size(probes).or.nmom<1)stop "gpu_chebyshev_moments_real_dev ERROR: moments must be (size(probes),nmom), nmom >= 1"
    if(present(self_moments))then
       if(size(self_moments)/=2*nmom-1)stop "gpu_chebyshev_moments_real_dev ERROR: self_moments must have 2*nmom-1 entries"
    endif
    plist=c_null_ptr
    do j=1,size(probes)
       if(probes(j)%sector_id/=handle_serial.or..not.c_associated(probes(j)%d))stop "gpu_chebyshev_moments_real_dev ERROR: a probe does not belong to the open sector"
       plist(j)=probes(j)%d
    enddo
    allocate(mom(max(size(probes),1),nmom),smom(2*nmom-1))      !(contiguous, whatever section the caller passed)
    call check(hxv_chebyshev_moments_real(handle,vin%d,int(size(probes),c_int32_t),plist,int(nmom,c_int32_t),a,b,mom,smom),"gpu_chebyshev_moments_real_dev")
    if(size(probes)>0)moments=mom
    if(present(self_moments))self_moments=smom
  end subroutine gpu_chebyshev_moments_real_dev

  !> gpu_chebyshev_apply_dev on REAL vectors (include/hxv.h, hxv_chebyshev_apply_real): a real H, a purely real vin, REAL coefficients.
  !! out has an imaginary part of exactly zero and is written only when the call succeeds.
  subroutine gpu_chebyshev_apply_real_dev(vin,coef,a,b,out,norm2)
    type(gpu_vector),intent(in)    :: vin
    real(8),intent(in)             :: coef(:)
    real(8),intent(in)             :: a,b
    type(gpu_vector),intent(inout) :: out
    real(8),intent(out),optional   :: norm2
    real(8),allocatable            :: cf(:)
    real(8)                        :: n2
    if(.not.c_associated(handle))stop "gpu_chebyshev_apply_real_dev ERROR: Hsector NOT set"
    if(vin%sector_id/=handle_serial.or..not.c_associated(vin%d))stop "gpu_chebyshev_apply_real_dev ERROR: the start vector does not belong to the open sector"
    if(size(coef)<1)stop "gpu_chebyshev_apply_real_dev ERROR: at least one coefficient"
    if(.not.c_associated(out%d))then
       call check(hxv_vector_alloc(handle,out%d),"gpu_chebyshev_apply_real_dev")
       call vec_born(out,out%d,.false.)
    endif
    if(out%sector_id/=handle_serial)stop "gpu_chebyshev_apply_real_dev ERROR: the output does not belong to the open sector"
    allocate(cf(size(coef))); cf=coef                           !(contiguous, whatever section the caller passed)
    n2=0d0
    call check(hxv_chebyshev_apply_real(handle,vin%d,int(size(coef),c_int32_t),cf,a,b,out%d,n2),"gpu_chebyshev_apply_real_dev")
    if(present(norm2))norm2=n2
  end subroutine gpu_chebyshev_apply_real_dev

  !> A seeded random device vector of the open sector (include/hxv.h, hxv_vector_random): components uniform in [-0.5,0.5), not
  !! normalised; real-valued (imaginary part exactly zero) unless complex_valued.  The same seed gives the same vector whatever the device
  !! row order or the rank split.  An empty vec is allocated on the open sector.
  subroutine gpu_vector_random_dev(seed,vec,complex_valued)
    integer(8),intent(in)          :: seed
    type(gpu_vector),intent(inout) :: vec
    logical,intent(in),optional    :: complex_valued
    integer(c_int32_t)             :: cv
    if(.not.c_associated(handle))stop "gpu_vector_random_dev ERROR: Hsector NOT set"
    if(.not.c_associated(vec%d))then
       call check(hxv_vector_alloc(handle,vec%d),"gpu_vector_random_dev")
       call vec_born(vec,vec%d,.false.)
    endif
    if(vec%sector_id/=handle_serial)stop "gpu_vector_random_dev ERROR: the vector does not belong to the open sector"
    cv=0; if(present(complex_valued))cv=merge(1,0,complex_valued)
    call check(hxv_vector_random(handle,int(seed,c_int64_t),cv,vec%d),"gpu_vector_random_dev")
  end subroutine gpu_vector_random_dev

  !> TWO gpu_sp_lanc_tridiag_probes_dev runs on one product per step (real H; include/hxv.h, hxv_lanczos_tridiag_pair_probes): the start
  !! vectors and the probes are REAL vectors of the open sector (c / c^dagger applied to a real ground state), the probes are shared by both
  !! runs -- orbitals i, i' of one spin with all c^dagger_j|gs> as probes.  overlaps_x(j,k) = <probes(j)|q_k> of run x, REAL
  !! (size(probes), size(alanc_x)): the imaginary parts the engine returns are exactly zero and are dropped here.  Columns of steps a run
  !! did not make are zero; nsteps_x = the steps done.  gpu_gf_from_probes takes cmplx(overlaps_x(:,1:nsteps_x),0d0,8).
  subroutine gpu_sp_lanc_tridiag_pair_probes_dev(vin_a,vin_b,probes,alanc_a,blanc_a,overlaps_a,alanc_b,blanc_b,overlaps_b,threshold,nsteps_a,nsteps_b)
    type(gpu_vector),intent(in)  :: vin_a,vin_b
    type(gpu_vector),intent(in)  :: probes(:)
    real(8),intent(inout)        :: alanc_a(:),blanc_a(:),alanc_b(:),blanc_b(:)
    real(8),intent(inout)        :: overlaps_a(:,:),overlaps_b(:,:)
    real(8),intent(in),optional  :: threshold
    integer,intent(out),optional :: nsteps_a,nsteps_b
    real(8)                      :: thr
    integer(c_int32_t)           :: na,nb
    type(c_ptr)                  :: plist(8)
    complex(8),allocatable       :: ova(:,:),ovb(:,:)
    integer                      :: j
    if(.not.c_associated(handle))stop "gpu_sp_lanc_tridiag_pair_probes_dev ERROR: Hsector NOT set"
    if(vin_a%sector_id/=handle_serial.or.vin_b%sector_id/=handle_serial.or..not.c_associated(vin_a%d).or..not.c_associated(vin_b%d))&
         stop "gpu_sp_lanc_tridiag_pair_probes_dev ERROR: the start vectors do not belong to the open sector"
    if(size(alanc_a)/=size(alanc_b))stop "gpu_sp_lanc_tridiag_pair_probes_dev ERROR: the two channels need equally long alanc/blanc"
    if(size(probes)>8)stop "gpu_sp_lanc_tridiag_pair_probes_dev ERROR: more than 8 probes"
    if(size(overlaps_a,1)/=size(probes).or.size(overlaps_a,2)/=size(alanc_a).or.size(blanc_a)/=size(alanc_a).or.&
         size(overlaps_b,1)/=size(probes).or.size(overlaps_b,2)/=size(alanc_b).or.size(blanc_b)/=size(alanc_b))&
         stop "gpu_sp_lanc_tridiag_pair_probes_dev ERROR: overlaps_x must be (size(probes),size(alanc_x)), blanc_x as long as alanc_x"
    plist=c_null_ptr
    do j=1,size(probes)
       if(probes(j)%sector_id/=handle_serial.or..not.c_associated(probes(j)%d))stop "gpu_sp_lanc_tridiag_pair_probes_dev ERROR: a probe does not belong to the open sector"
       plist(j)=probes(j)%d
    enddo
    thr=1d-12; if(present(threshold))thr=threshold
    allocate(ova(max(size(probes),1),size(alanc_a)),ovb(max(size(probes),1),size(alanc_b)))      !(contiguous, whatever section the caller passed)
    call check(hxv_lanczos_tridiag_pair_probes(handle,vin_a%d,vin_b%d,int(size(probes),c_int32_t),plist,int(size(alanc_a),c_int32_t),&
         alanc_a,blanc_a,ova,alanc_b,blanc_b,ovb,thr,na,nb),"gpu_sp_lanc_tridiag_pair_probes_dev")
    if(size(probes)>0)then
       overlaps_a=real(ova,8)
       overlaps_b=real(ovb,8)
    endif
    if(present(nsteps_a))nsteps_a=int(na)
    if(present(nsteps_b))nsteps_b=int(nb)
  end subroutine gpu_sp_lanc_tridiag_pair_probes_dev

  !> Poles and weights from one probes run (include/hxv.h, hxv_gf_from_probes; host code only, the engine's own tridiagonal QL): with
  !! alanc, blanc and overlaps(:,1:nsteps) of gpu_sp_lanc_tridiag_probes_dev and norm = |v| of the unnormalised start vector (sqrt of
  !! gpu_apply_ladder's norm2),   <probes(j)|(z - H)^-1|v> ~ sum_n weights(j,n) / (z - poles(n)),   n = 1..size(alanc).
  !! In the reference's conventions (add_to_lanczos_gf_normal, ED_GF_NORMAL.f90:915-975): de = poles(n) - Ei, a c^dagger channel (isign = +1)
  !! adds weights(j,n)/(z - de), a c channel (isign = -1) adds weights(j,n)/(z + de).
  subroutine gpu_gf_from_probes(alanc,blanc,overlaps,norm,poles,weights)
    real(8),intent(in)       :: alanc(:),blanc(:)
    complex(8),intent(in)    :: overlaps(:,:)
    real(8),intent(in)       :: norm
    real(8),intent(inout)    :: poles(:)
    complex(8),intent(inout) :: weights(:,:)
    real(8),allocatable      :: a(:),b(:)
    complex(8),allocatable   :: ov(:,:),w(:,:)
    integer                  :: n,np
    n=size(alanc); np=size(overlaps,1)
    if(size(blanc)/=n.or.size(overlaps,2)/=n.or.size(poles)/=n.or.size(weights,1)/=np.or.size(weights,2)/=n)&
         stop "gpu_gf_from_probes ERROR: alanc, blanc, poles of one length n; overlaps, weights (nprobes,n)"
    allocate(a(n),b(n),ov(max(np,1),n),w(max(np,1),n))  !(contiguous copies, whatever sections the caller passed)
    a=alanc; b=blanc; ov=(0d0,0d0); if(np>0)ov=overlaps
    call check(hxv_gf_from_probes(int(n,c_int32_t),a,b,int(np,c_int32_t),ov,norm,poles,w),"gpu_gf_from_probes")
    if(np>0)weights=w
  end subroutine gpu_gf_from_probes

  !> Density-type operators on a device vector of the OPEN sector (include/hxv.h, hxv_apply_density_ops): the start vectors of the two-particle
  !! stage (buildChi_impurity, ED_GREENS_FUNCTIONS.f90:68-106).  coef(is,1,a) / coef(is,2,a) are the coefficients of n_{is,up} / n_{is,dw}
  !! in operator a, is = iorb+(ilat-1)*Norb over the Nimp impurity orbitals (S^z_i: +1/2, -1/2 on is = i; n_i: 1, 1);
  !!     out(a) = (O_a - m_a) psi,   mean(a) = <psi|O_a|psi>/<psi|psi>,   m_a = mean(a) unless subtract_mean=.false.,   norm2(a) = <out(a)|out(a)>.
  !! Empty entries of out are allocated on the open sector.  chi_ab then takes one gpu_sp_lanc_tridiag_probes_dev run per b from out(b) with
  !! all out(:) as probes and gpu_gf_from_probes with norm = sqrt(norm2(b)):
  !!     chi_ab(z) = - sum_n [ weights(a,n)/(z - de_n) - conjg(weights(a,n))/(z + de_n) ],   de_n = poles(n) - E,   poles with |de_n| <= 1d-8 left out
  !! (the rounding ghosts of psi itself).  On a split sector psi and out are this rank's slabs and the call is collective.
  subroutine gpu_apply_density_ops_dev(psi,coef,out,mean,norm2,subtract_mean)
    type(gpu_vector),intent(in)    :: psi
    real(8),intent(in)             :: coef(:,:,:)
    type(gpu_vector),intent(inout) :: out(:)
    real(8),intent(inout)          :: mean(:),norm2(:)
    logical,intent(in),optional    :: subtract_mean
    real(8),allocatable            :: cf(:,:,:)
    real(8)                        :: m(8),n2(8)
    type(c_ptr)                    :: olist(8)
    integer(c_int32_t)             :: sub
    integer                        :: a,nops
    if(.not.c_associated(handle))stop "gpu_apply_density_ops_dev ERROR: Hsector NOT set"
    if(psi%sector_id/=handle_serial.or..not.c_associated(psi%d))stop "gpu_apply_density_ops_dev ERROR: the state does not belong to the open sector"
    nops=size(coef,3)
    if(nops<1.or.nops>8)stop "gpu_apply_density_ops_dev ERROR: 1 to 8 operators"
    if(size(coef,2)/=2.or.size(out)/=nops.or.size(mean)/=nops.or.size(norm2)/=nops)&
         stop "gpu_apply_density_ops_dev ERROR: coef is (Nimp,2,nops); out, mean, norm2 have nops entries"
    olist=c_null_ptr
    do a=1,nops
       if(.not.c_associated(out(a)%d))then
          call check(hxv_vector_alloc(handle,out(a)%d),"gpu_apply_density_ops_dev")
          call vec_born(out(a),out(a)%d,.false.)
       endif
       if(out(a)%sector_id/=handle_serial)stop "gpu_apply_density_ops_dev ERROR: an output does not belong to the open sector"
       olist(a)=out(a)%d
    enddo
    sub=1; if(present(subtract_mean))then; if(.not.subtract_mean)sub=0; endif
    allocate(cf(size(coef,1),2,nops)); cf=coef          !(contiguous, whatever section the caller passed)
    call check(hxv_apply_density_ops(handle,int(nops,c_int32_t),cf,sub,psi%d,olist,m,n2),"gpu_apply_density_ops_dev")
    mean=m(1:nops); norm2=n2(1:nops)
  end subroutine gpu_apply_density_ops_dev

  !> Operators that change both spin sectors at once (include/hxv.h, hxv_apply_spin_pair): the start vectors of the pair susceptibility
  !! (build_chi_pair, ED_GREENS_FUNCTIONS.f90:68-106) and of the transverse spin susceptibility,
  !!     out = sum_t coef(t) X_t Y_t psi,   X_t = c^dagger (create_up) or c on up orbital ipos_up(t),   Y_t the same on dw orbital ipos_dw(t),
  !! from psi's sector (kept open by gpu_keep_sector, as gpu_apply_ladder takes it) into the OPEN sector (nup+-1, ndw+-1); ipos = 1-based
  !! orbital position in the spin string, iorb+(ilat-1)*Norb for the impurity; 1 to 32 terms, summed in the order given; norm2 = <out|out>.
  !! The signs are those of two gpu_apply_ladder calls.  An empty out is allocated on the open sector.  chi_ab then takes, per operator, one
  !! gpu_sp_lanc_tridiag_probes_dev run in each neighbouring sector and gpu_gf_from_probes with norm = sqrt(norm2) (INTEGRATION.md section 4).
  !! Unsplit sectors only.
  subroutine gpu_apply_spin_pair_dev(psi,ipos_up,ipos_dw,coef,create_up,create_dw,out,norm2)
    type(gpu_vector),intent(in)    :: psi
    integer,intent(in)             :: ipos_up(:),ipos_dw(:)
    complex(8),intent(in)          :: coef(:)
    logical,intent(in)             :: create_up,create_dw
    type(gpu_vector),intent(inout) :: out
    real(8),intent(out)            :: norm2
    integer(c_int32_t)             :: ou(32),od(32),cu,cd
    real(8)                        :: cf(64)
    integer                        :: t,nterms
    if(.not.c_associated(handle))stop "gpu_apply_spin_pair_dev ERROR: Hsector NOT set (build the target sector first)"
    if(.not.vec_alive(psi))stop "gpu_apply_spin_pair_dev ERROR: empty source vector, or its sector was closed under it (gpu_keep_sector keeps it open)"
    nterms=size(coef)
    if(nterms<1.or.nterms>32)stop "gpu_apply_spin_pair_dev ERROR: 1 to 32 terms"
    if(size(ipos_up)/=nterms.or.size(ipos_dw)/=nterms)stop "gpu_apply_spin_pair_dev ERROR: ipos_up, ipos_dw and coef have one entry per term"
    if(.not.c_associated(out%d))then
       call check(hxv_vector_alloc(handle,out%d),"gpu_apply_spin_pair_dev")
       call vec_born(out,out%d,.false.)
    endif
    if(out%sector_id/=handle_serial)stop "gpu_apply_spin_pair_dev ERROR: the target vector does not belong to the open sector"
    do t=1,nterms
       ou(t)=int(ipos_up(t)-1,c_int32_t); od(t)=int(ipos_dw(t)-1,c_int32_t)
       cf(2*t-1)=dble(coef(t)); cf(2*t)=aimag(coef(t))
    enddo
    cu=0; if(create_up)cu=1
    cd=0; if(create_dw)cd=1
    call check(hxv_apply_spin_pair(psi%sector,handle,cu,cd,int(nterms,c_int32_t),ou,od,cf,psi%d,out%d,norm2),"gpu_apply_spin_pair_dev")
  end subroutine gpu_apply_spin_pair_dev

  !> One-body operators inside the OPEN sector (include/hxv.h, hxv_apply_one_body): the start vectors of the bond-order, current-current and
  !! inter-orbital exciton susceptibilities,
  !!     out = (O - m) psi,   O = sum_t coef(t) c^dagger_{ipos_to(t),s} c_{ipos_from(t),s},   s = ispin(t) (1 = up, 2 = dw),
  !!     mean = <psi|O|psi>/<psi|psi>,   m = mean unless subtract_mean=.false.,   norm2 = <out|out>;
  !! ipos = 1-based orbital position in the spin string, bath included, iorb+(ilat-1)*Norb for the impurity; ipos_to = ipos_from is the
  !! occupation; 1 to 32 terms, summed in the order given.  The signs are those of two gpu_apply_ladder calls.  An empty out is allocated
  !! on the open sector.  chi_ab then takes, per operator, gpu_sp_lanc_tridiag_probes_dev runs in the same sector and gpu_gf_from_probes
  !! with norm = sqrt(norm2) (INTEGRATION.md section 4).  Unsplit sectors only.
  subroutine gpu_apply_one_body_dev(psi,ispin,ipos_to,ipos_from,coef,out,mean,norm2,subtract_mean)
    type(gpu_vector),intent(in)    :: psi
    integer,intent(in)             :: ispin(:),ipos_to(:),ipos_from(:)
    complex(8),intent(in)          :: coef(:)
    type(gpu_vector),intent(inout) :: out
    complex(8),intent(out)         :: mean
    real(8),intent(out)            :: norm2
    logical,intent(in),optional    :: subtract_mean
    integer(c_int32_t)             :: sp(32),oi(32),oj(32),sub
    real(8)                        :: cf(64),m(2)
    integer                        :: t,nterms
    if(.not.c_associated(handle))stop "gpu_apply_one_body_dev ERROR: Hsector NOT set"
    if(psi%sector_id/=handle_serial.or..not.c_associated(psi%d))stop "gpu_apply_one_body_dev ERROR: the state does not belong to the open sector"
    nterms=size(coef)
    if(nterms<1.or.nterms>32)stop "gpu_apply_one_body_dev ERROR: 1 to 32 terms"
    if(size(ispin)/=nterms.or.size(ipos_to)/=nterms.or.size(ipos_from)/=nterms)&
         stop "gpu_apply_one_body_dev ERROR: ispin, ipos_to, ipos_from and coef have one entry per term"
    if(.not.c_associated(out%d))then
       call check(hxv_vector_alloc(handle,out%d),"gpu_apply_one_body_dev")
       call vec_born(out,out%d,.false.)
    endif
    if(out%sector_id/=handle_serial)stop "gpu_apply_one_body_dev ERROR: the output does not belong to the open sector"
    do t=1,nterms
       sp(t)=int(ispin(t)-1,c_int32_t); oi(t)=int(ipos_to(t)-1,c_int32_t); oj(t)=int(ipos_from(t)-1,c_int32_t)
       cf(2*t-1)=dble(coef(t)); cf(2*t)=aimag(coef(t))
    enddo
    sub=1; if(present(subtract_mean))then; if(.not.subtract_mean)sub=0; endif
    m=0d0
    call check(hxv_apply_one_body(handle,int(nterms,c_int32_t),sp,oi,oj,cf,sub,psi%d,out%d,m,norm2),"gpu_apply_one_body_dev")
    mean=cmplx(m(1),m(2),8)
  end subroutine gpu_apply_one_body_dev

  !> the vector in the reference's host layout (this rank's slab), when it is wanted there after all (e.g. state_list of ED_DIAG)
  subroutine gpu_vector_to_host(vect,v)
    type(gpu_vector),intent(in) :: vect
    complex(8),intent(inout)    :: v(:)
    if(.not.vec_alive(vect))stop "gpu_vector_to_host ERROR: empty vector, or its sector was closed under it"
    if(int(size(v),c_int64_t)/=hxv_vecdim(vect%sector))stop "gpu_vector_to_host ERROR: size(v) /= vecDim of the vector's sector"
    call check(hxv_vector_to_host(vect%sector,vect%d,v),"gpu_vector_to_host")
  end subroutine gpu_vector_to_host

  subroutine gpu_vector_from_host(v,vect)
    complex(8),intent(in)          :: v(:)
    type(gpu_vector),intent(inout) :: vect
    if(.not.c_associated(vect%d))then
       if(.not.c_associated(handle))stop "gpu_vector_from_host ERROR: Hsector NOT set"
       call check(hxv_vector_alloc(handle,vect%d),"gpu_vector_from_host")
       call vec_born(vect,vect%d,.false.)
    endif
    if(.not.vec_alive(vect))stop "gpu_vector_from_host ERROR: the vector's sector was closed under it"
    if(int(size(v),c_int64_t)/=hxv_vecdim(vect%sector))stop "gpu_vector_from_host ERROR: size(v) /= vecDim of the vector's sector"
    call check(hxv_vector_from_host(vect%sector,v,vect%d),"gpu_vector_from_host")
  end subroutine gpu_vector_from_host

  !> Any order: the allocation goes back when its last vector is freed, a kept sector is closed when its last vector is freed.
  subroutine gpu_free_vector(vect)
    type(gpu_vector),intent(inout) :: vect
    integer                        :: ia,is
    if(c_associated(vect%d))then
       is=ref_find(sector_refs,vect%sector_id)
       ia=ref_find(alloc_refs,vect%alloc_id)
       if(is==0.or.ia==0)stop "gpu_free_vector ERROR: not a live device vector (a copy of one that was freed already?)"
       alloc_refs(ia)%n=alloc_refs(ia)%n-1
       if(alloc_refs(ia)%n==0)then
          if(.not.sector_refs(is)%dead)call check(hxv_vector_free(vect%sector,vect%base),"gpu_free_vector")
          alloc_refs(ia)%id=0
       endif
       sector_refs(is)%n=sector_refs(is)%n-1
       if(sector_refs(is)%n==0)then
          if(sector_refs(is)%kept.and..not.sector_refs(is)%dead)then
             if(vect%sector_id==handle_serial)then; handle=c_null_ptr; handle_serial=0; endif   !(kept sectors are never the open one; belt and braces)
             call check(hxv_destroy(vect%sector),"gpu_free_vector")
          endif
          sector_refs(is)%id=0; sector_refs(is)%kept=.false.; sector_refs(is)%dead=.false.
       endif
    endif
    vect%d=c_null_ptr; vect%sector=c_null_ptr; vect%base=c_null_ptr; vect%owns_sector=.false.; vect%view=.false.; vect%sector_id=0; vect%alloc_id=0
  end subroutine gpu_free_vector

  !> Sectors (engine handles) opened and not yet closed, process-wide (include/hxv.h: hxv_live_handles): a host program's leak check.
  function gpu_live_sectors() result(n)
    integer(8) :: n
    n=hxv_live_handles()
  end function gpu_live_sectors

  !> Vector-sized bytes the engine has moved over PCIe for a sector since it was opened (include/hxv.h: hxv_stats): the open sector,
  !! or the kept sector of `vect`.
  subroutine gpu_pcie_bytes(h2d,d2h,vect)
    integer(8),intent(out)               :: h2d,d2h
    type(gpu_vector),intent(in),optional :: vect
    type(hxv_stats)                      :: st
    type(c_ptr)                          :: hh
    hh=handle
    if(present(vect))then
       if(.not.vec_alive(vect))stop "gpu_pcie_bytes ERROR: empty vector, or its sector was closed under it"
       hh=vect%sector
    endif
    if(.not.c_associated(hh))stop "gpu_pcie_bytes ERROR: no sector"
    call check(hxv_get_stats(hh,st),"gpu_pcie_bytes")
    h2d=st%h2d_bytes; d2h=st%d2h_bytes
  end subroutine gpu_pcie_bytes

  !> build_Hv_sector from the reference's OWN stored matrices (ED_HAMILTONIAN_SPARSE_HxV.f90:40-152 has built spH0ups(1), spH0dws(1),
  !! spH0d): flatten each sparse_matrix_csr (ED_SPARSE_MATRIX.f90:13-30) row by row --
  !!     rowptr(1)=0; do i=1,Nrow; rowptr(i+1)=rowptr(i)+sparse%row(i)%Size
  !!                              cols(rowptr(i)+1:rowptr(i+1))=sparse%row(i)%cols; vals(...)=sparse%row(i)%vals; enddo
  !! (columns stay 1-based, as sp_insert_element stores them) -- and the diagonal spH0d as its local rows, one value per row.
  subroutine gpu_build_Hv_sector_from_csr(DimUp,DimDw,up_rowptr,up_cols,up_vals,dw_rowptr,dw_cols,dw_vals,diag,MpiRank,MpiSize,device)
    integer,intent(in)          :: DimUp,DimDw
    integer(8),intent(in)       :: up_rowptr(:),dw_rowptr(:)     ![DimUp+1], [DimDw+1], 0-based offsets
    integer,intent(in)          :: up_cols(:),dw_cols(:)         !1-based columns
    complex(8),intent(in)       :: up_vals(:),dw_vals(:),diag(:) !diag: mpiQdw*DimUp local rows
    integer,intent(in)          :: MpiRank,MpiSize
    integer,intent(in),optional :: device
    integer                     :: dev
    if(c_associated(handle))stop "gpu_build_Hv_sector_from_csr ERROR: a sector is already open"
    if(size(up_rowptr)/=DimUp+1.or.size(dw_rowptr)/=DimDw+1)stop "gpu_build_Hv_sector_from_csr ERROR: rowptr sizes"
    dev=0;if(present(device))dev=device
    call check(hxv_create_from_csr(int(DimUp,c_int32_t),int(DimDw,c_int32_t),int(up_rowptr,c_int64_t),int(up_cols,c_int32_t),up_vals,&
         int(dw_rowptr,c_int64_t),int(dw_cols,c_int32_t),dw_vals,diag,int(MpiRank,c_int32_t),int(MpiSize,c_int32_t),int(dev,c_int32_t),handle),&
         "gpu_build_Hv_sector_from_csr")
    call sector_opened()
    call check(hxv_set_option(handle,"eigh_degenerate"//c_null_char,merge(1_c_int64_t,0_c_int64_t,gpu_eigh_degenerate)),"gpu_build_Hv_sector_from_csr")
  end subroutine gpu_build_Hv_sector_from_csr

  !> stored elements of H_up (which=1) / H_dw (which=2) of the open sector
  function gpu_sector_nnz(which) result(nnz)
    integer,intent(in) :: which
    integer(8)         :: nnz
    if(.not.c_associated(handle))stop "gpu_sector_nnz ERROR: Hsector NOT set"
    nnz=hxv_nnz(handle,int(which-1,c_int32_t))
  end function gpu_sector_nnz

  !> H_up (which=1) / H_dw (which=2) of the open sector as the engine built it, flattened like spH0ups(1) / spH0dws(1) would be for
  !! gpu_build_Hv_sector_from_csr: rowptr(DimSigma+1) 0-based offsets, cols 1-based, vals complex
  subroutine gpu_get_sector_csr(which,rowptr,cols,vals)
    integer,intent(in)       :: which
    integer(8),intent(out)   :: rowptr(:)
    integer,intent(out)      :: cols(:)
    complex(8),intent(out)   :: vals(:)
    integer(c_int64_t),allocatable :: rp(:)
    integer(c_int32_t),allocatable :: cl(:)
    if(.not.c_associated(handle))stop "gpu_get_sector_csr ERROR: Hsector NOT set"
    if(int(size(cols),8)<hxv_nnz(handle,int(which-1,c_int32_t)).or.size(vals)<size(cols))stop "gpu_get_sector_csr ERROR: cols / vals too short"
    allocate(rp(size(rowptr)),cl(size(cols)))
    call check(hxv_get_csr(handle,int(which-1,c_int32_t),rp,cl,vals),"gpu_get_sector_csr")
    rowptr=rp; cols=cl
    deallocate(rp,cl)
  end subroutine gpu_get_sector_csr

  !> the (real) diagonal of the open sector, local rows -- spH0d's values
  subroutine gpu_get_sector_diag(diag)
    real(8),intent(out) :: diag(:)
    if(.not.c_associated(handle))stop "gpu_get_sector_diag ERROR: Hsector NOT set"
    if(int(size(diag),c_int64_t)/=hxv_vecdim(handle))stop "gpu_get_sector_diag ERROR: size(diag) /= vecDim"
    call check(hxv_get_diag(handle,diag),"gpu_get_sector_diag")
  end subroutine gpu_get_sector_diag

  !> spH0nd (Jx, Jp; ED_VARS_GLOBAL.f90:145, sparse/H_non_local.f90:23-98) of a sector opened from stored matrices: the LOCAL rows with the
  !! reference's GLOBAL 1-based columns, flattened like the others.
  subroutine gpu_set_nonlocal_csr(rowptr,cols,vals)
    integer(8),intent(in) :: rowptr(:)
    integer,intent(in)    :: cols(:)
    complex(8),intent(in) :: vals(:)
    if(.not.c_associated(handle))stop "gpu_set_nonlocal_csr ERROR: Hsector NOT set"
    call check(hxv_set_nonlocal_csr(handle,int(rowptr,c_int64_t),int(cols,c_int32_t),vals),"gpu_set_nonlocal_csr")
  end subroutine gpu_set_nonlocal_csr

  !> MpiComm-first forms: the call text of the reference's MpiStatus=T branches compiles against these unchanged,
  !!   call sp_eigh(MpiComm,spHtimesV_p,eig_values,eig_basis,Nblock,Nitermax,tol=lanc_tolerance,iverbose=(ed_verbose>3))   ED_DIAG.f90:152-156
  !!   call sp_lanc_eigh(MpiComm,spHtimesV_p,eig_values(1),eig_basis(:,1),Nitermax,iverbose=...,threshold=lanc_tolerance)    ED_DIAG.f90:176-177
  !!   call sp_lanc_tridiag(MpiComm,spHtimesV_p,vvloc,alfa_,beta_)                                                            ED_GF_NORMAL.f90:215
  !! with vectors = this rank's slab (vecDim_Hv_sector elements).  MpiComm is the reference's integer communicator.
  subroutine gpu_sp_eigh_mpi(MpiComm,MatVec,eval,evec,Nblock,Nitermax,tol,iverbose)
    integer,intent(in)          :: MpiComm
    interface
       subroutine MatVec(Nloc,v,Hv)
         integer                    :: Nloc
         complex(8),dimension(Nloc) :: v,Hv
       end subroutine MatVec
    end interface
    real(8),intent(inout)       :: eval(:)
    complex(8),intent(inout)    :: evec(:,:)
    integer,intent(in),optional :: Nblock,Nitermax
    real(8),intent(in),optional :: tol
    logical,intent(in),optional :: iverbose
    call gpu_sp_eigh_serial(MatVec,eval,evec,Nblock,Nitermax,tol,iverbose)
  end subroutine gpu_sp_eigh_mpi

  subroutine gpu_sp_lanc_eigh_mpi(MpiComm,MatVec,egs,vect,Nitermax,iverbose,threshold)
    integer,intent(in)          :: MpiComm
    interface
       subroutine MatVec(Nloc,v,Hv)
         integer                    :: Nloc
         complex(8),dimension(Nloc) :: v,Hv
       end subroutine MatVec
    end interface
    real(8),intent(inout)       :: egs
    complex(8),intent(inout)    :: vect(:)
    integer,intent(in)          :: Nitermax
    logical,intent(in),optional :: iverbose
    real(8),intent(in),optional :: threshold
    call gpu_sp_lanc_eigh_serial(MatVec,egs,vect,Nitermax,iverbose,threshold)
  end subroutine gpu_sp_lanc_eigh_mpi

  subroutine gpu_sp_lanc_tridiag_mpi(MpiComm,MatVec,vin,alanc,blanc,threshold)
    integer,intent(in)          :: MpiComm
    interface
       subroutine MatVec(Nloc,v,Hv)
         integer                    :: Nloc
         complex(8),dimension(Nloc) :: v,Hv
       end subroutine MatVec
    end interface
    complex(8),intent(inout)    :: vin(:)
    real(8),intent(inout)       :: alanc(:),blanc(:)
    real(8),intent(in),optional :: threshold
    call gpu_sp_lanc_tridiag_serial(MatVec,vin,alanc,blanc,threshold)
  end subroutine gpu_sp_lanc_tridiag_mpi

  !> One state of state_list (ED_OBSERVABLES.f90:110-140) into the module's summed record: vect is a device vector (gpu_sp_eigh_dev /
  !! gpu_sp_lanc_eigh_dev) on its own sector -- the open one, or one kept open for it by gpu_keep_sector, as gpu_apply_ladder takes it --
  !! peso the reference's weight exp(-beta(Ei-Egs))/zeta_function.  accumulate=.false. starts a new sum (the first state), .true. adds to
  !! it.  On a split sector every rank calls it with its slab and holds the global record.
  subroutine gpu_observables_dev(vect,peso,accumulate)
    type(gpu_vector),intent(in) :: vect
    real(8),intent(in)          :: peso
    logical,intent(in)          :: accumulate
    integer(c_int64_t)          :: n
    if(.not.vec_alive(vect))stop "gpu_observables_dev ERROR: empty vector, or its sector was closed under it (gpu_keep_sector keeps it open)"
    n=hxv_obs_record_elems(vect%sector)
    if(n<=0)stop "gpu_observables_dev ERROR: the open sector has no impurity record (Nimp > 10, or no basis maps)"
    if(accumulate)then
       if(.not.allocated(obs_record))stop "gpu_observables_dev ERROR: accumulate=.true. before a first state"
       if(size(obs_record,kind=c_int64_t)/=n)stop "gpu_observables_dev ERROR: the record of this sector belongs to another model"
    else
       if(allocated(obs_record))deallocate(obs_record)
       allocate(obs_record(n))
    endif
    call check(hxv_observables_accumulate(vect%sector,vect%d,real(peso,c_double),merge(1_c_int32_t,0_c_int32_t,accumulate),obs_record),&
         "gpu_observables_dev")
  end subroutine gpu_observables_dev

  !> The named quantities of the summed record (hxv_observables_derive), shaped like the reference's: ed_dens, ed_dens_up, ed_dens_dw,
  !! ed_docc (Nlat,Norb), ed_Eknot, ed_Epot (Ehartree included, ED_OBSERVABLES.f90:434), ed_Ehartree, ed_Dust, ed_Dund and
  !! single_particle_density_matrix (Nlat,Nlat,Nspin,Nspin,Norb,Norb); magz, sz2, n2, s2tot optionally.  The model inputs are the module
  !! globals the reference has in scope (ED_INPUT_VARS.f90:13-16,129-135,164; impHloc ED_VARS_GLOBAL.f90:119).  Ehartree's constant term
  !! uses Uloc(iorb), not the reference's Uloc(is) (:399, which reads past Norb): include/hxv.h.
  subroutine gpu_get_observables(Nlat,Norb,Nspin,impHloc,Uloc,Ust,Jh,hfmode,dens,dens_up,dens_dw,docc,Eknot,Epot,Ehartree,Dust,Dund,&
       spdm,magz,sz2,n2,s2tot)
    integer,intent(in)                      :: Nlat,Norb,Nspin
    complex(8),intent(in),target,contiguous :: impHloc(:,:,:,:,:,:)   ![Nlat,Nlat,Nspin,Nspin,Norb,Norb]
    real(8),intent(in)                      :: Uloc(5),Ust,Jh
    logical,intent(in)                      :: hfmode
    real(8),intent(out)                     :: dens(Nlat,Norb),dens_up(Nlat,Norb),dens_dw(Nlat,Norb),docc(Nlat,Norb)
    real(8),intent(out)                     :: Eknot,Epot,Ehartree,Dust,Dund
    complex(8),intent(out)                  :: spdm(Nlat,Nlat,Nspin,Nspin,Norb,Norb)
    real(8),intent(out),optional            :: magz(Nlat,Norb),sz2(Nlat,Nlat,Norb,Norb),n2(Nlat,Nlat,Norb,Norb),s2tot(Nlat)
    type(hxv_model)                         :: m
    real(c_double),allocatable              :: out(:)
    integer(c_int64_t)                      :: n
    integer                                 :: k,lo,llo,i
    if(.not.allocated(obs_record))stop "gpu_get_observables ERROR: no state recorded (gpu_observables_dev)"
    m%nlat=Nlat; m%norb=Norb; m%nspin=Nspin; m%nbath=0
    m%hfmode=0; if(hfmode)m%hfmode=1
    m%reserved=0
    m%uloc=Uloc
    m%ust=Ust; m%jh=Jh; m%jx=0d0; m%jp=0d0; m%xmu=0d0
    m%imphloc=c_loc(impHloc); m%hbath=c_null_ptr; m%vbath=c_null_ptr
    if(size(obs_record,kind=c_int64_t)/=4_c_int64_t**(Nlat*Norb)+4_c_int64_t*(Nlat*Norb)**2)&
         stop "gpu_get_observables ERROR: the recorded sector belongs to another model"
    n=hxv_obs_derived_elems(m)
    if(n<=0)stop "gpu_get_observables ERROR: unsupported model (Nimp <= 10, Norb <= 5)"
    allocate(out(n))
    call check(hxv_observables_derive(m,obs_record,out),"gpu_get_observables")
    lo=Nlat*Norb; llo=lo*lo
    k=0
    dens   =reshape(out(k+1:k+lo),[Nlat,Norb]); k=k+lo
    dens_up=reshape(out(k+1:k+lo),[Nlat,Norb]); k=k+lo
    dens_dw=reshape(out(k+1:k+lo),[Nlat,Norb]); k=k+lo
    docc   =reshape(out(k+1:k+lo),[Nlat,Norb]); k=k+lo
    if(present(magz))magz=reshape(out(k+1:k+lo),[Nlat,Norb]); k=k+lo
    if(present(sz2))sz2=reshape(out(k+1:k+llo),[Nlat,Nlat,Norb,Norb]); k=k+llo
    if(present(n2))n2=reshape(out(k+1:k+llo),[Nlat,Nlat,Norb,Norb]); k=k+llo
    if(present(s2tot))s2tot=out(k+1:k+Nlat); k=k+Nlat
    Eknot=out(k+1); Epot=out(k+2); Ehartree=out(k+3); Dust=out(k+4); Dund=out(k+5); k=k+5
    spdm=reshape([(cmplx(out(k+2*i-1),out(k+2*i),kind=8),i=1,llo*Nspin*Nspin)],[Nlat,Nlat,Nspin,Nspin,Norb,Norb])
    deallocate(out)
  end subroutine gpu_get_observables

  !> One state of state_list (ED_OBSERVABLES.f90:489-503) into the module's summed cluster density matrix rho_imp = Tr_bath |psi><psi|
  !! (:514-575, without the eigenvector on the host): vect and peso as gpu_observables_dev takes them.  accumulate=.false. starts a new sum
  !! (the first state; cluster_density_matrix=zero of :486), .true. adds to it.  On a split sector every rank calls it with its slab and
  !! holds the global matrix.
  subroutine gpu_cluster_dm_dev(vect,peso,accumulate)
    type(gpu_vector),intent(in) :: vect
    real(8),intent(in)          :: peso
    logical,intent(in)          :: accumulate
    integer(c_int64_t)          :: n
    if(.not.vec_alive(vect))stop "gpu_cluster_dm_dev ERROR: empty vector, or its sector was closed under it (gpu_keep_sector keeps it open)"
    n=hxv_cluster_dm_elems(vect%sector)
    if(n<=0)stop "gpu_cluster_dm_dev ERROR: the open sector has no cluster density matrix (Nimp > 5, or no basis maps)"
    if(accumulate)then
       if(.not.allocated(cdm_sum))stop "gpu_cluster_dm_dev ERROR: accumulate=.true. before a first state"
       if(size(cdm_sum,kind=c_int64_t)/=n)stop "gpu_cluster_dm_dev ERROR: the matrix of this sector belongs to another model"
    else
       if(allocated(cdm_sum))deallocate(cdm_sum)
       allocate(cdm_sum(n))
    endif
    call check(hxv_cluster_dm_accumulate(vect%sector,vect%d,real(peso,c_double),merge(1_c_int32_t,0_c_int32_t,accumulate),cdm_sum),&
         "gpu_cluster_dm_dev")
  end subroutine gpu_cluster_dm_dev

  !> One state of state_list into rdm, the reduced density matrix of the impurity orbitals orbital_mask(ilat,jorb) names -- the mask
  !! ed_get_reduced_density_matrix_single takes (ED_IO/get_reduced_dm.f90:68-212) -- computed from the device-resident vector instead of a
  !! masked trace of cluster_density_matrix, so for any Nimp: rdm(4**Nred,4**Nred), 1 <= Nred <= 4, element (io,jo) with
  !! io = (iREDup + 2**Nred*iREDdw) + 1 (:146).  vect and peso as gpu_cluster_dm_dev takes them.  accumulate=.false. overwrites rdm (the first
  !! state), .true. adds peso * (this state's matrix) to it.  fermi_sign absent or .false.: the reference's numbers (its sign factor, :148, is
  !! +1 on every pair that contributes: a plain partial trace); .true.: the matrix with the Jordan-Wigner sign of the subset, whose spectrum is
  !! physical for any mask (include/hxv.h).  On a split sector every rank calls it with its slab and holds the global matrix.
  subroutine gpu_reduced_dm_dev(vect,orbital_mask,peso,rdm,accumulate,fermi_sign)
    type(gpu_vector),intent(in) :: vect
    logical,intent(in)          :: orbital_mask(:,:)   !(Nlat,Norb)
    real(8),intent(in)          :: peso
    complex(8),intent(inout)    :: rdm(:,:)
    logical,intent(in)          :: accumulate
    logical,intent(in),optional :: fermi_sign
    real(c_double),allocatable  :: buf(:)
    integer(c_int32_t)          :: mask,fs
    integer(c_int64_t)          :: n
    integer                     :: ilat,jorb,i,j,m
    if(.not.vec_alive(vect))stop "gpu_reduced_dm_dev ERROR: empty vector, or its sector was closed under it (gpu_keep_sector keeps it open)"
    if(size(orbital_mask)>32)stop "gpu_reduced_dm_dev ERROR: orbital_mask has more than 32 entries"
    mask=0
    do ilat=1,size(orbital_mask,1)
       do jorb=1,size(orbital_mask,2)
          if(orbital_mask(ilat,jorb))mask=ibset(mask,jorb+(ilat-1)*size(orbital_mask,2)-1)
       enddo
    enddo
    fs=0; if(present(fermi_sign))fs=merge(1_c_int32_t,0_c_int32_t,fermi_sign)
    n=hxv_reduced_dm_elems(vect%sector,mask)
    if(n<=0)stop "gpu_reduced_dm_dev ERROR: no reduced density matrix for this mask on the open sector (1 to 4 orbitals inside Nimp; basis maps)"
    m=size(rdm,1)
    if(size(rdm,2)/=m.or.2_c_int64_t*int(m,c_int64_t)*m/=n)stop "gpu_reduced_dm_dev ERROR: rdm is not (4**Nred,4**Nred)"
    allocate(buf(n))
    if(accumulate)then
       do j=1,m
          do i=1,m
             buf(2*(i+m*(j-1))-1)=dble(rdm(i,j))
             buf(2*(i+m*(j-1)))=aimag(rdm(i,j))
          enddo
       enddo
    endif
    call check(hxv_reduced_dm_accumulate(vect%sector,vect%d,mask,fs,real(peso,c_double),merge(1_c_int32_t,0_c_int32_t,accumulate),buf),&
         "gpu_reduced_dm_dev")
    do j=1,m
       do i=1,m
          rdm(i,j)=cmplx(buf(2*(i+m*(j-1))-1),buf(2*(i+m*(j-1))),kind=8)
       enddo
    enddo
    deallocate(buf)
  end subroutine gpu_reduced_dm_dev

  !> The summed matrix into the reference's cluster_density_matrix(4**Nimp,4**Nimp) (ED_VARS_GLOBAL.f90), as is: element (io,jo),
  !! io = (IimpUp + 2**Nimp*IimpDw) + 1 (ED_OBSERVABLES.f90:561-566).
  subroutine gpu_get_cluster_dm(cdm)
    complex(8),intent(out) :: cdm(:,:)
    integer                :: i,j,n
    if(.not.allocated(cdm_sum))stop "gpu_get_cluster_dm ERROR: no state recorded (gpu_cluster_dm_dev)"
    n=size(cdm,1)
    if(size(cdm,2)/=n.or.2_c_int64_t*int(n,c_int64_t)*n/=size(cdm_sum,kind=c_int64_t))&
         stop "gpu_get_cluster_dm ERROR: cdm is not (4**Nimp,4**Nimp) of the recorded sector"
    do j=1,n
       do i=1,n
          cdm(i,j)=cmplx(cdm_sum(2*(i+n*(j-1))-1),cdm_sum(2*(i+n*(j-1))),kind=8)
       enddo
    enddo
  end subroutine gpu_get_cluster_dm

end module ED_HAMILTONIAN_GPU_HXV
