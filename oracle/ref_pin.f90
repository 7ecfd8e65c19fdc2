! ref_pin.f90 -- TEST INFRASTRUCTURE ONLY: runs the REFERENCE's own Hamiltonian loop nests, unmodified, on a model written by Python.
!
! The reference keeps its hot path as include fragments (ED_HAMILTONIAN/sparse/*.f90, ED_HAMILTONIAN/direct/*.f90): loop nests without a
! USE line that read every name from the scope that includes them.  This file declares such a scope (ours) and includes the eight
! fragments at compile time (flang -I <reference tree>); it holds no reference text beyond the include file names.
!
!   ref_pin INPUT STREAMS [HV]
!
!   INPUT    (little-endian stream) int32 Nlat,Norb,Nspin,Nbath,hfmode,nup,ndw,DimUp,DimDw; real64 Uloc(5),Ust,Jh,Jx,Jp,xmu;
!            complex impHloc(Nlat,Nlat,Nspin,Nspin,Norb,Norb), complex hbath(...,Nbath), real64 vbath(Nlat,Nspin,Norb,Nbath) as hxv_model
!            lays them out; int32 map_up(DimUp), map_dw(DimDw); complex vin(DimUp*DimDw)
!   STREAMS  output A: one 28-byte record per sp_insert_element call of the four sparse fragments, IN CALL ORDER:
!            int32 matrix id (1 spH0d, 2 spH0nd, 3 spH0ups(1), 4 spH0dws(1)), int32 i, int32 j, real64 Re, real64 Im.  Nothing is summed.
!   HV       output B (only when named): Hv of directMatVec_main's body: Hv = 0, local, up, dw, non-local if Jhflag; complex(Dim).
!
! OURS, NOT THE REFERENCE'S (pinned only by the Jordan-Wigner test of tests/test_oracle_pins.py): bdecomp, c, cdg, binary_search,
! imp_state_index, iup_index, idw_index, the getBathStride table -- written from their definitions -- and the recorder that stands
! where the reference's sparse-matrix type is.
module ref_pin_scope
  implicit none
  complex(8), parameter :: zero = (0d0, 0d0)
  ! model inputs
  integer :: Nlat, Norb, Nspin, Nbath, Ns
  logical :: hfmode, Jhflag
  real(8) :: Uloc(5), Ust, Jh, Jx, Jp, xmu
  complex(8), allocatable :: impHloc(:, :, :, :, :, :), hbath_in(:, :, :, :, :, :, :)
  real(8), allocatable :: vbath_in(:, :, :, :)
  integer, allocatable :: getBathStride(:, :, :)
  ! sector
  type sector_map
    integer, allocatable :: map(:)
  end type sector_map
  type(sector_map) :: Hs(2)
  integer :: DimUp, DimDw, Dim
  ! serial run: MpiStatus = F, every row local
  logical :: MpiStatus = .false.
  integer :: MpiComm = 0, MpiIstart, MpiIend, mpiIshift = 0
  ! the recorder
  type recorder
    integer :: id = 0
  end type recorder
  type(recorder) :: spH0d, spH0nd, spH0ups(1), spH0dws(1)
  integer :: rec_unit = -1
  interface sp_insert_element
    module procedure record_element, record_element_comm
  end interface sp_insert_element
contains

  subroutine record_element(sparse, value, i, j)
    type(recorder), intent(in) :: sparse
    complex(8), intent(in) :: value
    integer, intent(in) :: i, j
    write (rec_unit) int(sparse%id, 4), int(i, 4), int(j, 4), real(value, 8), aimag(value)
  end subroutine record_element

  subroutine record_element_comm(comm, sparse, value, i, j)
    integer, intent(in) :: comm
    type(recorder), intent(in) :: sparse
    complex(8), intent(in) :: value
    integer, intent(in) :: i, j
    error stop "ref_pin: the communicator form of sp_insert_element is never reached with MpiStatus = F"
  end subroutine record_element_comm

  ! occupation numbers of the Ntot lowest bits of i, lowest bit first
  function bdecomp(i, Ntot) result(ivec)
    integer, intent(in) :: i, Ntot
    integer :: ivec(Ntot), l
    do l = 1, Ntot
      ivec(l) = ibits(i, l - 1, 1)
    end do
  end function bdecomp

  ! fermionic sign of acting on orbital pos: parity of the occupied orbitals below it
  pure function below_sign(pos, state) result(s)
    integer, intent(in) :: pos, state
    real(8) :: s
    s = 1d0
    if (poppar(iand(state, ishft(1, pos - 1) - 1)) == 1) s = -1d0
  end function below_sign

  subroutine c(pos, in, out, fsgn)
    integer, intent(in) :: pos, in
    integer, intent(inout) :: out
    real(8), intent(inout) :: fsgn
    if (.not. btest(in, pos - 1)) error stop "ref_pin: c on an empty orbital"
    fsgn = below_sign(pos, in)
    out = ibclr(in, pos - 1)
  end subroutine c

  subroutine cdg(pos, in, out, fsgn)
    integer, intent(in) :: pos, in
    integer, intent(inout) :: out
    real(8), intent(inout) :: fsgn
    if (btest(in, pos - 1)) error stop "ref_pin: cdg on an occupied orbital"
    fsgn = below_sign(pos, in)
    out = ibset(in, pos - 1)
  end subroutine cdg

  ! 1-based position of value in the ascending array a, 0 when absent
  function binary_search(a, value) result(pos)
    integer, intent(in) :: a(:), value
    integer :: pos, lo, hi, mid
    pos = 0
    lo = 1
    hi = size(a)
    do while (lo <= hi)
      mid = lo + (hi - lo)/2
      if (a(mid) == value) then
        pos = mid
        return
      else if (a(mid) < value) then
        lo = mid + 1
      else
        hi = mid - 1
      end if
    end do
  end function binary_search

  integer function imp_state_index(ilat, iorb)
    integer, intent(in) :: ilat, iorb
    imp_state_index = iorb + (ilat - 1)*Norb
  end function imp_state_index

  ! i = iup + (idw-1)*DimUp, both 1-based
  integer function iup_index(i, DimUp_)
    integer, intent(in) :: i, DimUp_
    iup_index = mod(i - 1, DimUp_) + 1
  end function iup_index

  integer function idw_index(i, DimUp_)
    integer, intent(in) :: i, DimUp_
    idw_index = (i - 1)/DimUp_ + 1
  end function idw_index

  ! ---- the scope of ed_buildh_main: output A ----
  subroutine run_sparse_fragments()
    integer :: i, iup, idw, j, jup, jdw, mup, mdw
    integer :: ilat, jlat, iorb, jorb, ispin, ibath, is, js
    integer :: k1, k2, k3, k4, ialfa, ibeta
    real(8) :: sg1, sg2, sg3, sg4
    complex(8) :: htmp
    logical :: Jcondition
    integer, dimension(Ns) :: ibup, ibdw
    integer, dimension(Nlat, Norb) :: Nup, Ndw
    real(8), dimension(Nlat, Nspin, Norb, Nbath) :: diag_hybr, bath_diag
    complex(8), dimension(Nlat, Nlat, Nspin, Nspin, Norb, Norb, Nbath) :: Hbath_reconstructed
    call derive_bath(diag_hybr, bath_diag, Hbath_reconstructed)
    Nup = 0
    Ndw = 0
    include "ED_HAMILTONIAN/sparse/H_local.f90"
    if (Jhflag) then
      include "ED_HAMILTONIAN/sparse/H_non_local.f90"
    end if
    include "ED_HAMILTONIAN/sparse/H_up.f90"
    include "ED_HAMILTONIAN/sparse/H_dw.f90"
  end subroutine run_sparse_fragments

  ! ---- the scope of directMatVec_main: output B ----
  subroutine run_direct_fragments(Nloc, vin, Hv)
    integer :: Nloc
    complex(8), dimension(Nloc) :: vin, Hv
    integer :: i, iup, idw, j, jup, jdw, mup, mdw
    integer :: ilat, jlat, iorb, jorb, ispin, ibath, is, js
    integer :: k1, k2, k3, k4, ialfa, ibeta
    real(8) :: sg1, sg2, sg3, sg4
    complex(8) :: htmp
    logical :: Jcondition
    integer, dimension(Ns) :: ibup, ibdw
    integer, dimension(Nlat, Norb) :: Nup, Ndw
    real(8), dimension(Nlat, Nspin, Norb, Nbath) :: diag_hybr, bath_diag
    complex(8), dimension(Nlat, Nlat, Nspin, Nspin, Norb, Norb, Nbath) :: Hbath_reconstructed
    ! direct/HxV_local.f90 bounds its ilat bath loop by size(bath_diag,3) = Norb: past bath_diag when Nlat < Norb
    if (Nbath > 0 .and. Nlat < Norb) error stop "ref_pin: the direct fragment indexes past bath_diag when Nlat < Norb and Nbath > 0"
    call derive_bath(diag_hybr, bath_diag, Hbath_reconstructed)
    Hv = zero
    include "ED_HAMILTONIAN/direct/HxV_local.f90"
    include "ED_HAMILTONIAN/direct/HxV_up.f90"
    include "ED_HAMILTONIAN/direct/HxV_dw.f90"
    if (Jhflag) then
      include "ED_HAMILTONIAN/direct/HxV_non_local.f90"
    end if
  end subroutine run_direct_fragments

  ! diagonal hybridisation and the REAL part of the bath diagonal, as both callers of the fragments derive them
  subroutine derive_bath(diag_hybr, bath_diag, Hbath_reconstructed)
    real(8), dimension(Nlat, Nspin, Norb, Nbath) :: diag_hybr, bath_diag
    complex(8), dimension(Nlat, Nlat, Nspin, Nspin, Norb, Norb, Nbath) :: Hbath_reconstructed
    integer :: ibath, ilat, ispin, iorb
    diag_hybr = 0d0
    bath_diag = 0d0
    do ibath = 1, Nbath
      Hbath_reconstructed(:, :, :, :, :, :, ibath) = hbath_in(:, :, :, :, :, :, ibath)
      do ilat = 1, Nlat
        do ispin = 1, Nspin
          do iorb = 1, Norb
            diag_hybr(ilat, ispin, iorb, ibath) = vbath_in(ilat, ispin, iorb, ibath)
            bath_diag(ilat, ispin, iorb, ibath) = real(Hbath_reconstructed(ilat, ilat, ispin, ispin, iorb, iorb, ibath), 8)
          end do
        end do
      end do
    end do
  end subroutine derive_bath
end module ref_pin_scope

program ref_pin
  use ref_pin_scope
  implicit none
  character(len=4096) :: f_in, f_streams, f_hv
  integer(4) :: head(9)
  integer(4), allocatable :: m4(:)
  real(8) :: par(10)
  complex(8), allocatable :: vin(:), Hv(:)
  integer :: u, ilat, iorb, ibath, sec_nup, sec_ndw
  if (command_argument_count() < 2) error stop "usage: ref_pin INPUT STREAMS [HV]"
  call get_command_argument(1, f_in)
  call get_command_argument(2, f_streams)
  open (newunit=u, file=trim(f_in), access="stream", form="unformatted", status="old", action="read")
  read (u) head
  Nlat = head(1); Norb = head(2); Nspin = head(3); Nbath = head(4); hfmode = head(5) /= 0
  sec_nup = head(6); sec_ndw = head(7); DimUp = head(8); DimDw = head(9)
  read (u) par
  Uloc = par(1:5); Ust = par(6); Jh = par(7); Jx = par(8); Jp = par(9); xmu = par(10)
  Ns = Nlat*Norb*(Nbath + 1)
  if (Ns > 30) error stop "ref_pin: Ns > 30"
  Dim = DimUp*DimDw
  allocate (impHloc(Nlat, Nlat, Nspin, Nspin, Norb, Norb), hbath_in(Nlat, Nlat, Nspin, Nspin, Norb, Norb, Nbath))
  allocate (vbath_in(Nlat, Nspin, Norb, Nbath), Hs(1)%map(DimUp), Hs(2)%map(DimDw), vin(Dim), Hv(Dim), m4(max(DimUp, DimDw)))
  read (u) impHloc
  if (Nbath > 0) read (u) hbath_in
  if (Nbath > 0) read (u) vbath_in
  read (u) m4(1:DimUp)
  Hs(1)%map = m4(1:DimUp)
  read (u) m4(1:DimDw)
  Hs(2)%map = m4(1:DimDw)
  read (u) vin
  close (u)
  if (popcnt(Hs(1)%map(1)) /= sec_nup .or. popcnt(Hs(2)%map(1)) /= sec_ndw) error stop "ref_pin: sector maps do not match (nup,ndw)"
  Jhflag = .false.
  if (Norb > 1 .and. (Jx /= 0d0 .or. Jp /= 0d0)) Jhflag = .true.
  allocate (getBathStride(Nlat, Norb, Nbath))
  do ibath = 1, Nbath
    do ilat = 1, Nlat
      do iorb = 1, Norb
        getBathStride(ilat, iorb, ibath) = ibath*Nlat*Norb + imp_state_index(ilat, iorb)
      end do
    end do
  end do
  MpiIstart = 1
  MpiIend = Dim
  spH0d%id = 1; spH0nd%id = 2; spH0ups(1)%id = 3; spH0dws(1)%id = 4
  open (newunit=rec_unit, file=trim(f_streams), access="stream", form="unformatted", status="replace", action="write")
  call run_sparse_fragments()
  close (rec_unit)
  if (command_argument_count() >= 3) then
    call get_command_argument(3, f_hv)
    call run_direct_fragments(Dim, vin, Hv)
    open (newunit=u, file=trim(f_hv), access="stream", form="unformatted", status="replace", action="write")
    write (u) Hv
    close (u)
  end if
end program ref_pin
