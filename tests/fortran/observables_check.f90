!> Test host for tests/test_gpu_fortran_observables.py: reads a model and a sector from the raw file named on the command line (stream I/O,
!! written by the test), finds the ground state on the device (gpu_sp_eigh_dev), records it (gpu_observables_dev) and prints what
!! gpu_get_observables returns.  Input, in order: Nlat, Norb, Nspin, Nbath, nup, ndw, hfmode (int32); impHloc, Hbath (complex(8));
!! Vbath, Uloc(5), Ust, Jh, Jx, Jp, xmu (real(8)), all in the reference's Fortran array order.
program observables_check
  use ED_HAMILTONIAN_GPU_HXV
  implicit none
  integer(4)                 :: Nlat,Norb,Nspin,Nbath,nup,ndw,ihf
  complex(8),allocatable     :: impHloc(:,:,:,:,:,:),Hbath(:,:,:,:,:,:,:),spdm(:,:,:,:,:,:)
  real(8),allocatable        :: Vbath(:,:,:,:),dens(:,:),dens_up(:,:),dens_dw(:,:),docc(:,:)
  real(8)                    :: Uloc(5),Ust,Jh,Jx,Jp,xmu,Eknot,Epot,Ehartree,Dust,Dund,e(1)
  type(gpu_vector)           :: ev(1)
  character(len=512)         :: path
  integer                    :: u
  call get_command_argument(1,path)
  open(newunit=u,file=trim(path),access="stream",form="unformatted",status="old")
  read(u)Nlat,Norb,Nspin,Nbath,nup,ndw,ihf
  allocate(impHloc(Nlat,Nlat,Nspin,Nspin,Norb,Norb),Hbath(Nlat,Nlat,Nspin,Nspin,Norb,Norb,max(Nbath,1)),Vbath(Nlat,Nspin,Norb,max(Nbath,1)))
  read(u)impHloc
  if(Nbath>0)read(u)Hbath(:,:,:,:,:,:,1:Nbath)
  if(Nbath>0)read(u)Vbath(:,:,:,1:Nbath)
  read(u)Uloc,Ust,Jh,Jx,Jp,xmu
  close(u)
  allocate(dens(Nlat,Norb),dens_up(Nlat,Norb),dens_dw(Nlat,Norb),docc(Nlat,Norb),spdm(Nlat,Nlat,Nspin,Nspin,Norb,Norb))
  call gpu_build_Hv_sector(Nlat,Norb,Nspin,Nbath,nup,ndw,impHloc,Hbath(:,:,:,:,:,:,1:Nbath),Vbath(:,:,:,1:Nbath),Uloc,Ust,Jh,Jx,Jp,xmu,&
       ihf/=0,0,1)
  call gpu_sp_eigh_dev(e,ev,20,512,tol=1d-14)
  call gpu_observables_dev(ev(1),1d0,.false.)
  call gpu_get_observables(Nlat,Norb,Nspin,impHloc,Uloc,Ust,Jh,ihf/=0,dens,dens_up,dens_dw,docc,Eknot,Epot,Ehartree,Dust,Dund,spdm)
  call gpu_free_vector(ev(1))
  call gpu_delete_Hv_sector()
  write(*,"(A,ES24.16)")"E0= ",e(1)
  write(*,"(A,*(ES24.16))")"dens= ",dens
  write(*,"(A,*(ES24.16))")"docc= ",docc
  write(*,"(A,ES24.16)")"Eknot= ",Eknot
  write(*,"(A,ES24.16)")"Epot= ",Epot
end program observables_check
