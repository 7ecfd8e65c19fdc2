!> Test host for tests/test_gpu_fortran_chebyshev.py: reads a model and a sector (nup,ndw) from the raw file named on the command line (stream
!! I/O, written by the test, the format of one_body_check.f90), followed by the window a, b, the number of coefficients and the complex
!! coefficients of a Chebyshev series.  Finds the ground state on the device (gpu_sp_lanc_eigh_dev), makes the start vector
!! v = c^+_{1,up} c_{2,up}|gs> inside the sector (gpu_apply_one_body_dev, no mean subtracted) and runs
!!   - gpu_chebyshev_moments_dev from v with the probes (gs, v): nmom = 12 moments per probe and the 23 self-moments,
!!   - gpu_chebyshev_apply_dev on v with the coefficients read: out, its norm2, and <gs|out>, <v|out> as the order-0 moments of out.
!! Prints them; frees everything and stops unless no sector is left open.
program chebyshev_check
  use ED_HAMILTONIAN_GPU_HXV
  implicit none
  integer,parameter          :: nmom=12
  integer(4)                 :: Nlat,Norb,Nspin,Nbath,nup,ndw,ihf,ncoef
  complex(8),allocatable     :: impHloc(:,:,:,:,:,:),Hbath(:,:,:,:,:,:,:),coef(:)
  real(8),allocatable        :: Vbath(:,:,:,:)
  real(8)                    :: Uloc(5),Ust,Jh,Jx,Jp,xmu,e0,a,b,smom(2*nmom-1),hop_norm2,norm2
  complex(8)                 :: moments(2,nmom),ov(2,1),hop_mean
  type(gpu_vector)           :: gs,v,out,probes(2)
  character(len=512)         :: path
  integer                    :: u
  complex(8),parameter       :: one=(1d0,0d0)
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
  close(u)
  call gpu_build_Hv_sector(Nlat,Norb,Nspin,Nbath,nup,ndw,impHloc,Hbath(:,:,:,:,:,:,1:Nbath),Vbath(:,:,:,1:Nbath),Uloc,Ust,Jh,Jx,Jp,xmu,&
       ihf/=0,0,1)
  call gpu_sp_lanc_eigh_dev(e0,gs,512,threshold=1d-14)
  call gpu_apply_one_body_dev(gs,[1],[1],[2],[one],v,hop_mean,hop_norm2,subtract_mean=.false.)
  probes(1)=gs; probes(2)=v
  moments=(0d0,0d0); smom=0d0
  call gpu_chebyshev_moments_dev(v,probes,a,b,moments,smom)
  call gpu_chebyshev_apply_dev(v,coef,a,b,out,norm2)
  ov=(0d0,0d0)
  call gpu_chebyshev_moments_dev(out,probes,a,b,ov)
  call gpu_free_vector(out)
  call gpu_free_vector(v)
  call gpu_free_vector(gs)
  call gpu_delete_Hv_sector()
  if(gpu_live_sectors()/=0)stop "chebyshev_check ERROR: a sector is still open"
  write(*,"(A,ES24.16)")"E0= ",e0
  write(*,"(A,*(ES24.16))")"mom_re= ",dble(moments)
  write(*,"(A,*(ES24.16))")"mom_im= ",aimag(moments)
  write(*,"(A,*(ES24.16))")"self= ",smom
  write(*,"(A,*(ES24.16))")"norm2= ",norm2
  write(*,"(A,*(ES24.16))")"ov= ",dble(ov),aimag(ov)
  write(*,"(A,I0)")"live_sectors= ",gpu_live_sectors()
end program chebyshev_check
