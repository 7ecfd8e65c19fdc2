!> Test host for tests/test_gpu_fortran_cluster_dm.py: reads a model and a sector from the raw file named on the command line (stream I/O,
!! written by the test, the format of observables_check.f90), finds the ground state on the device (gpu_sp_eigh_dev), records its cluster
!! density matrix (gpu_cluster_dm_dev) and prints, from what gpu_get_cluster_dm returns, the trace, the purity and the block of the impurity
!! configurations with one particle per spin (io = 2**i + 2**Nimp * 2**j, off-diagonal elements included).
program cluster_dm_check
  use ED_HAMILTONIAN_GPU_HXV
  implicit none
  integer(4)                 :: Nlat,Norb,Nspin,Nbath,nup,ndw,ihf
  complex(8),allocatable     :: impHloc(:,:,:,:,:,:),Hbath(:,:,:,:,:,:,:),cdm(:,:)
  real(8),allocatable        :: Vbath(:,:,:,:)
  real(8)                    :: Uloc(5),Ust,Jh,Jx,Jp,xmu,e(1),tr,purity
  type(gpu_vector)           :: ev(1)
  character(len=512)         :: path
  integer,allocatable        :: idx(:)
  integer                    :: u,Nimp,n,i,j
  call get_command_argument(1,path)
  open(newunit=u,file=trim(path),access="stream",form="unformatted",status="old")
  read(u)Nlat,Norb,Nspin,Nbath,nup,ndw,ihf
  allocate(impHloc(Nlat,Nlat,Nspin,Nspin,Norb,Norb),Hbath(Nlat,Nlat,Nspin,Nspin,Norb,Norb,max(Nbath,1)),Vbath(Nlat,Nspin,Norb,max(Nbath,1)))
  read(u)impHloc
  if(Nbath>0)read(u)Hbath(:,:,:,:,:,:,1:Nbath)
  if(Nbath>0)read(u)Vbath(:,:,:,1:Nbath)
  read(u)Uloc,Ust,Jh,Jx,Jp,xmu
  close(u)
  Nimp=Nlat*Norb
  n=4**Nimp
  allocate(cdm(n,n),idx(Nimp*Nimp))
  call gpu_build_Hv_sector(Nlat,Norb,Nspin,Nbath,nup,ndw,impHloc,Hbath(:,:,:,:,:,:,1:Nbath),Vbath(:,:,:,1:Nbath),Uloc,Ust,Jh,Jx,Jp,xmu,&
       ihf/=0,0,1)
  call gpu_sp_eigh_dev(e,ev,20,512,tol=1d-14)
  call gpu_cluster_dm_dev(ev(1),1d0,.false.)
  call gpu_get_cluster_dm(cdm)
  call gpu_free_vector(ev(1))
  call gpu_delete_Hv_sector()
  tr=0d0
  do i=1,n
     tr=tr+dble(cdm(i,i))
  enddo
  purity=dble(sum(cdm*transpose(cdm)))
  do j=0,Nimp-1
     do i=0,Nimp-1
        idx(1+i+Nimp*j)=2**i+2**Nimp*2**j+1
     enddo
  enddo
  write(*,"(A,ES24.16)")"E0= ",e(1)
  write(*,"(A,ES24.16)")"trace= ",tr
  write(*,"(A,ES24.16)")"purity= ",purity
  write(*,"(A,*(ES24.16))")"block_re= ",dble(cdm(idx,idx))
  write(*,"(A,*(ES24.16))")"block_im= ",aimag(cdm(idx,idx))
end program cluster_dm_check
