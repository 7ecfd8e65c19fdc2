!> Test host for tests/test_gpu_fortran_reduced_dm.py: reads a model and a sector from the raw file named on the command line (stream I/O,
!! written by the test, the format of cluster_dm_check.f90), finds the ground state on the device (gpu_sp_eigh_dev) and calls
!! gpu_reduced_dm_dev with a one-site mask (site 1: every orbital of it), with the mask of the impurity bits {0,1}, and with the latter in
!! the Fermi-sign convention; prints the trace, the purity and the matrix of each.
program reduced_dm_check
  use ED_HAMILTONIAN_GPU_HXV
  implicit none
  integer(4)                 :: Nlat,Norb,Nspin,Nbath,nup,ndw,ihf
  complex(8),allocatable     :: impHloc(:,:,:,:,:,:),Hbath(:,:,:,:,:,:,:),rdm(:,:)
  real(8),allocatable        :: Vbath(:,:,:,:)
  logical,allocatable        :: mask(:,:)
  real(8)                    :: Uloc(5),Ust,Jh,Jx,Jp,xmu,e(1)
  type(gpu_vector)           :: ev(1)
  character(len=512)         :: path
  integer                    :: u,b
  call get_command_argument(1,path)
  open(newunit=u,file=trim(path),access="stream",form="unformatted",status="old")
  read(u)Nlat,Norb,Nspin,Nbath,nup,ndw,ihf
  allocate(impHloc(Nlat,Nlat,Nspin,Nspin,Norb,Norb),Hbath(Nlat,Nlat,Nspin,Nspin,Norb,Norb,max(Nbath,1)),Vbath(Nlat,Nspin,Norb,max(Nbath,1)))
  read(u)impHloc
  if(Nbath>0)read(u)Hbath(:,:,:,:,:,:,1:Nbath)
  if(Nbath>0)read(u)Vbath(:,:,:,1:Nbath)
  read(u)Uloc,Ust,Jh,Jx,Jp,xmu
  close(u)
  allocate(mask(Nlat,Norb))
  call gpu_build_Hv_sector(Nlat,Norb,Nspin,Nbath,nup,ndw,impHloc,Hbath(:,:,:,:,:,:,1:Nbath),Vbath(:,:,:,1:Nbath),Uloc,Ust,Jh,Jx,Jp,xmu,&
       ihf/=0,0,1)
  call gpu_sp_eigh_dev(e,ev,20,512,tol=1d-14)
  write(*,"(A,ES24.16)")"E0= ",e(1)
  !one site
  mask=.false.; mask(1,:)=.true.
  allocate(rdm(4**Norb,4**Norb))
  call gpu_reduced_dm_dev(ev(1),mask,1d0,rdm,.false.)
  call show("site")
  deallocate(rdm)
  !impurity bits 0 and 1: b = jorb + (ilat-1)*Norb - 1
  mask=.false.
  do b=0,1
     mask(b/Norb+1,mod(b,Norb)+1)=.true.
  enddo
  allocate(rdm(16,16))
  call gpu_reduced_dm_dev(ev(1),mask,1d0,rdm,.false.)
  call show("pair")
  !the same in two halves and in the other convention
  call gpu_reduced_dm_dev(ev(1),mask,0.25d0,rdm,.false.,fermi_sign=.true.)
  call gpu_reduced_dm_dev(ev(1),mask,0.75d0,rdm,.true.,fermi_sign=.true.)
  call show("fermi")
  call gpu_free_vector(ev(1))
  call gpu_delete_Hv_sector()
contains
  subroutine show(tag)
    character(len=*),intent(in) :: tag
    real(8)                     :: tr
    integer                     :: i
    tr=0d0
    do i=1,size(rdm,1)
       tr=tr+dble(rdm(i,i))
    enddo
    write(*,"(A,ES24.16)")tag//"_trace= ",tr
    write(*,"(A,ES24.16)")tag//"_purity= ",dble(sum(rdm*transpose(rdm)))
    write(*,"(A,*(ES24.16))")tag//"_re= ",dble(rdm)
    write(*,"(A,*(ES24.16))")tag//"_im= ",aimag(rdm)
  end subroutine show
end program reduced_dm_check
