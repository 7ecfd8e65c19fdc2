!> Test host for tests/test_gpu_fortran_pair_probes.py: reads a model, a sector (nup,ndw) and nvec = 2 + nprobes real vectors of that sector
!! from the raw file named on the command line (stream I/O, written by the test: the header of probes_check.f90, then nprobes, Dim and the
!! vectors as complex(8) in the reference's layout), uploads them (gpu_vector_from_host) and runs ONE paired tridiagonalisation from the
!! first two with the others as probes of both (gpu_sp_lanc_tridiag_pair_probes_dev).  Prints the steps done, alanc, blanc and the real
!! overlaps of each run with every digit; frees everything and stops unless no sector is left open.
program pair_probes_check
  use ED_HAMILTONIAN_GPU_HXV
  implicit none
  integer,parameter          :: nlanc=30
  integer(4)                 :: Nlat,Norb,Nspin,Nbath,nup,ndw,ihf,nprobes,dim
  complex(8),allocatable     :: impHloc(:,:,:,:,:,:),Hbath(:,:,:,:,:,:,:),vec(:)
  real(8),allocatable        :: Vbath(:,:,:,:),ova(:,:),ovb(:,:)
  real(8)                    :: Uloc(5),Ust,Jh,Jx,Jp,xmu,alanc_a(nlanc),blanc_a(nlanc),alanc_b(nlanc),blanc_b(nlanc)
  type(gpu_vector)           :: va,vb
  type(gpu_vector),allocatable :: p(:)
  character(len=512)         :: path
  character(len=16)          :: key
  integer                    :: u,na,nb,j
  call get_command_argument(1,path)
  open(newunit=u,file=trim(path),access="stream",form="unformatted",status="old")
  read(u)Nlat,Norb,Nspin,Nbath,nup,ndw,ihf
  allocate(impHloc(Nlat,Nlat,Nspin,Nspin,Norb,Norb),Hbath(Nlat,Nlat,Nspin,Nspin,Norb,Norb,max(Nbath,1)),Vbath(Nlat,Nspin,Norb,max(Nbath,1)))
  read(u)impHloc
  if(Nbath>0)read(u)Hbath(:,:,:,:,:,:,1:Nbath)
  if(Nbath>0)read(u)Vbath(:,:,:,1:Nbath)
  read(u)Uloc,Ust,Jh,Jx,Jp,xmu
  read(u)nprobes,dim
  call gpu_build_Hv_sector(Nlat,Norb,Nspin,Nbath,nup,ndw,impHloc,Hbath(:,:,:,:,:,:,1:Nbath),Vbath(:,:,:,1:Nbath),Uloc,Ust,Jh,Jx,Jp,xmu,&
       ihf/=0,0,1)
  allocate(vec(dim),p(nprobes),ova(nprobes,nlanc),ovb(nprobes,nlanc))
  read(u)vec
  call gpu_vector_from_host(vec,va)
  read(u)vec
  call gpu_vector_from_host(vec,vb)
  do j=1,nprobes
     read(u)vec
     call gpu_vector_from_host(vec,p(j))
  enddo
  close(u)
  alanc_a=0d0; blanc_a=0d0; alanc_b=0d0; blanc_b=0d0; ova=7d0; ovb=7d0
  call gpu_sp_lanc_tridiag_pair_probes_dev(va,vb,p,alanc_a,blanc_a,ova,alanc_b,blanc_b,ovb,nsteps_a=na,nsteps_b=nb)
  call gpu_free_vector(va)
  call gpu_free_vector(vb)
  do j=1,nprobes
     call gpu_free_vector(p(j))
  enddo
  call gpu_delete_Hv_sector()
  if(gpu_live_sectors()/=0)stop "pair_probes_check ERROR: a sector is still open"
  write(*,"(A,I0)")"nsteps_a= ",na
  write(*,"(A,I0)")"nsteps_b= ",nb
  write(*,"(A,*(ES25.16E3))")"alanc_a= ",alanc_a
  write(*,"(A,*(ES25.16E3))")"blanc_a= ",blanc_a
  write(*,"(A,*(ES25.16E3))")"alanc_b= ",alanc_b
  write(*,"(A,*(ES25.16E3))")"blanc_b= ",blanc_b
  do j=1,nprobes
     write(key,"(A,I0,A)")"ov_a",j,"= "
     write(*,"(A,*(ES25.16E3))")trim(key)//" ",ova(j,:)
     write(key,"(A,I0,A)")"ov_b",j,"= "
     write(*,"(A,*(ES25.16E3))")trim(key)//" ",ovb(j,:)
  enddo
  write(*,"(A,I0)")"live_sectors= ",gpu_live_sectors()
end program pair_probes_check
