!> Test host for tests/test_gpu_fortran_twin.py: reads a model and a sector (nup,ndw) from the raw file named on the command line (stream I/O,
!! written by the test, the format of observables_check.f90), finds the ground state of that sector on the device (gpu_sp_eigh_dev), keeps
!! the sector open for it, opens the twin sector (ndw,nup), maps the state into it (gpu_twin_vector) and tridiagonalises from there
!! (gpu_sp_lanc_tridiag_dev): for a spin-symmetric model the twin is an eigenstate, so alanc(1) is the ground-state energy again.  Prints E0,
!! alanc(1) and the first 16 amplitudes of the twin's host copy; frees everything and stops unless no sector is left open.
program twin_check
  use ED_HAMILTONIAN_GPU_HXV
  implicit none
  integer(4)                 :: Nlat,Norb,Nspin,Nbath,nup,ndw,ihf
  complex(8),allocatable     :: impHloc(:,:,:,:,:,:),Hbath(:,:,:,:,:,:,:),v(:)
  real(8),allocatable        :: Vbath(:,:,:,:)
  real(8)                    :: Uloc(5),Ust,Jh,Jx,Jp,xmu,e(1),alanc(4),blanc(4)
  type(gpu_vector)           :: ev(1),tw
  character(len=512)         :: path
  integer                    :: u,n
  call get_command_argument(1,path)
  open(newunit=u,file=trim(path),access="stream",form="unformatted",status="old")
  read(u)Nlat,Norb,Nspin,Nbath,nup,ndw,ihf
  allocate(impHloc(Nlat,Nlat,Nspin,Nspin,Norb,Norb),Hbath(Nlat,Nlat,Nspin,Nspin,Norb,Norb,max(Nbath,1)),Vbath(Nlat,Nspin,Norb,max(Nbath,1)))
  read(u)impHloc
  if(Nbath>0)read(u)Hbath(:,:,:,:,:,:,1:Nbath)
  if(Nbath>0)read(u)Vbath(:,:,:,1:Nbath)
  read(u)Uloc,Ust,Jh,Jx,Jp,xmu
  close(u)
  call gpu_build_Hv_sector(Nlat,Norb,Nspin,Nbath,nup,ndw,impHloc,Hbath(:,:,:,:,:,:,1:Nbath),Vbath(:,:,:,1:Nbath),Uloc,Ust,Jh,Jx,Jp,xmu,&
       ihf/=0,0,1)
  call gpu_sp_eigh_dev(e,ev,20,512,tol=1d-14)
  call gpu_keep_sector(ev(1))
  call gpu_build_Hv_sector(Nlat,Norb,Nspin,Nbath,ndw,nup,impHloc,Hbath(:,:,:,:,:,:,1:Nbath),Vbath(:,:,:,1:Nbath),Uloc,Ust,Jh,Jx,Jp,xmu,&
       ihf/=0,0,1)
  call gpu_twin_vector(ev(1),tw)
  alanc=0d0; blanc=0d0
  call gpu_sp_lanc_tridiag_dev(tw,alanc,blanc)
  n=gpu_vecDim_Hv_sector()
  allocate(v(n))
  call gpu_vector_to_host(tw,v)
  call gpu_free_vector(tw)
  call gpu_delete_Hv_sector()
  call gpu_free_vector(ev(1))
  if(gpu_live_sectors()/=0)stop "twin_check ERROR: a sector is still open"
  write(*,"(A,ES24.16)")"E0= ",e(1)
  write(*,"(A,ES24.16)")"alanc1= ",alanc(1)
  write(*,"(A,*(ES24.16))")"amp_re= ",dble(v(1:min(16,n)))
  write(*,"(A,*(ES24.16))")"amp_im= ",aimag(v(1:min(16,n)))
  write(*,"(A,I0)")"live_sectors= ",gpu_live_sectors()
end program twin_check
