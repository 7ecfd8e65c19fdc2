!> Test host for tests/test_gpu_fortran_chebyshev_real.py: reads a model and a sector (nup,ndw) from the raw file named on the command line
!! (stream I/O, written by the test, the format of chebyshev_check.f90), followed by the window a, b, the number of coefficients, the REAL
!! coefficients of a Chebyshev series and a seed.  Makes the start vector v and a second vector p on the device (gpu_vector_random_dev, seeds
!! seed and seed+1, real-valued) and runs
!!   - gpu_chebyshev_moments_real_dev from v with the probes (p, v): nmom = 12 real moments per probe and the 23 self-moments,
!!   - gpu_chebyshev_apply_real_dev on v with the coefficients read: out, its norm2, and <p|out>, <v|out> as the order-0 moments of out.
!! Prints them; frees everything and stops unless no sector is left open.
program chebyshev_real_check
  use ED_HAMILTONIAN_GPU_HXV
  implicit none
  integer,parameter          :: nmom=12
  integer(4)                 :: Nlat,Norb,Nspin,Nbath,nup,ndw,ihf,ncoef
  integer(8)                 :: seed
  complex(8),allocatable     :: impHloc(:,:,:,:,:,:),Hbath(:,:,:,:,:,:,:)
  real(8),allocatable        :: Vbath(:,:,:,:),coef(:)
  real(8)                    :: Uloc(5),Ust,Jh,Jx,Jp,xmu,a,b,smom(2*nmom-1),norm2
  real(8)                    :: moments(2,nmom),ov(2,1)
  type(gpu_vector)           :: p,v,out,probes(2)
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
  read(u)a,b
  read(u)ncoef
  allocate(coef(ncoef))
  read(u)coef
  read(u)seed
  close(u)
  call gpu_build_Hv_sector(Nlat,Norb,Nspin,Nbath,nup,ndw,impHloc,Hbath(:,:,:,:,:,:,1:Nbath),Vbath(:,:,:,1:Nbath),Uloc,Ust,Jh,Jx,Jp,xmu,&
       ihf/=0,0,1)
  call gpu_vector_random_dev(seed,v)
  call gpu_vector_random_dev(seed+1_8,p,complex_valued=.false.)
  probes(1)=p; probes(2)=v
  moments=0d0; smom=0d0
  call gpu_chebyshev_moments_real_dev(v,probes,a,b,moments,smom)
  call gpu_chebyshev_apply_real_dev(v,coef,a,b,out,norm2)
  ov=0d0
  call gpu_chebyshev_moments_real_dev(out,probes,a,b,ov)
  call gpu_free_vector(out)
  call gpu_free_vector(v)
  call gpu_free_vector(p)
  call gpu_delete_Hv_sector()
  if(gpu_live_sectors()/=0)stop "chebyshev_real_check ERROR: a sector is still open"
  write(*,"(A,*(ES24.16))")"mom= ",moments
  write(*,"(A,*(ES24.16))")"self= ",smom
  write(*,"(A,*(ES24.16))")"norm2= ",norm2
  write(*,"(A,*(ES24.16))")"ov= ",ov
  write(*,"(A,I0)")"live_sectors= ",gpu_live_sectors()
end program chebyshev_real_check
