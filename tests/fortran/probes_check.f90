!> Test host for tests/test_gpu_fortran_probes.py: reads a model and the ground state's sector (nup,ndw) from the raw file named on the command
!! line (stream I/O, written by the test, the format of twin_check.f90), finds the ground state on the device (gpu_sp_lanc_eigh_dev), keeps its
!! sector, opens (nup+1,ndw), builds v = c^dagger_{1,up}|gs> and p = c^dagger_{2,up}|gs> there (gpu_apply_ladder) and runs ONE
!! tridiagonalisation from v with p as probe (gpu_sp_lanc_tridiag_probes_dev); gpu_gf_from_probes turns it into the poles and weights of
!! <p|(z - H)^-1|v>, the particle part of G_01.  Prints E0, norm2, the steps done, poles and weights; frees everything and stops unless no sector
!! is left open.
program probes_check
  use ED_HAMILTONIAN_GPU_HXV
  implicit none
  integer,parameter          :: nlanc=30
  integer(4)                 :: Nlat,Norb,Nspin,Nbath,nup,ndw,ihf
  complex(8),allocatable     :: impHloc(:,:,:,:,:,:),Hbath(:,:,:,:,:,:,:)
  real(8),allocatable        :: Vbath(:,:,:,:)
  real(8)                    :: Uloc(5),Ust,Jh,Jx,Jp,xmu,e0,alanc(nlanc),blanc(nlanc),poles(nlanc),n2v,n2p
  complex(8)                 :: overlaps(1,nlanc),weights(1,nlanc)
  type(gpu_vector)           :: gs,v,p(1)
  character(len=512)         :: path
  integer                    :: u,ns
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
  call gpu_sp_lanc_eigh_dev(e0,gs,512,threshold=1d-14)
  call gpu_keep_sector(gs)
  call gpu_build_Hv_sector(Nlat,Norb,Nspin,Nbath,nup+1,ndw,impHloc,Hbath(:,:,:,:,:,:,1:Nbath),Vbath(:,:,:,1:Nbath),Uloc,Ust,Jh,Jx,Jp,xmu,&
       ihf/=0,0,1)
  call gpu_apply_ladder(gs,1,1,.true.,v,n2v)
  call gpu_apply_ladder(gs,2,1,.true.,p(1),n2p)
  alanc=0d0; blanc=0d0; overlaps=(0d0,0d0)
  call gpu_sp_lanc_tridiag_probes_dev(v,p,alanc,blanc,overlaps,nsteps=ns)
  poles=0d0; weights=(0d0,0d0)
  call gpu_gf_from_probes(alanc(1:ns),blanc(1:ns),overlaps(:,1:ns),sqrt(n2v),poles(1:ns),weights(:,1:ns))
  call gpu_free_vector(v)
  call gpu_free_vector(p(1))
  call gpu_delete_Hv_sector()
  call gpu_free_vector(gs)
  if(gpu_live_sectors()/=0)stop "probes_check ERROR: a sector is still open"
  write(*,"(A,ES24.16)")"E0= ",e0
  write(*,"(A,ES24.16)")"norm2= ",n2v
  write(*,"(A,I0)")"nsteps= ",ns
  write(*,"(A,*(ES24.16))")"poles= ",poles(1:ns)
  write(*,"(A,*(ES24.16))")"w_re= ",dble(weights(1,1:ns))
  write(*,"(A,*(ES24.16))")"w_im= ",aimag(weights(1,1:ns))
  write(*,"(A,I0)")"live_sectors= ",gpu_live_sectors()
end program probes_check
