!> Test host for tests/test_gpu_fortran_chi.py: reads a model and the ground state's sector (nup,ndw) from the raw file named on the command
!! line (stream I/O, written by the test, the format of probes_check.f90), finds the ground state on the device (gpu_sp_lanc_eigh_dev), builds
!! dS^z_a|gs> for the two impurity sites in ONE gpu_apply_density_ops_dev call and computes chi_spin(i nu_n), n = 0, 1, 5, at beta = 50 from one
!! gpu_sp_lanc_tridiag_probes_dev run per column + gpu_gf_from_probes.  Prints E0, the means, the norms and chi; frees everything and stops
!! unless no sector is left open.
program chi_check
  use ED_HAMILTONIAN_GPU_HXV
  implicit none
  integer,parameter          :: nlanc=200,nimp=2,nfreq=3
  real(8),parameter          :: beta=50d0,pi=3.141592653589793238d0,cutoff=1d-8
  integer,parameter          :: ifreq(nfreq)=[0,1,5]
  integer(4)                 :: Nlat,Norb,Nspin,Nbath,nup,ndw,ihf
  complex(8),allocatable     :: impHloc(:,:,:,:,:,:),Hbath(:,:,:,:,:,:,:)
  real(8),allocatable        :: Vbath(:,:,:,:)
  real(8)                    :: Uloc(5),Ust,Jh,Jx,Jp,xmu,e0,alanc(nlanc),blanc(nlanc),poles(nlanc),coef(nimp,2,nimp),mean(nimp),norm2(nimp),de
  complex(8)                 :: overlaps(nimp,nlanc),weights(nimp,nlanc),chi(nfreq,nimp,nimp),z
  type(gpu_vector)           :: gs,dv(nimp)
  character(len=512)         :: path
  integer                    :: u,ns,a,b,n,k
  call get_command_argument(1,path)
  open(newunit=u,file=trim(path),access="stream",form="unformatted",status="old")
  read(u)Nlat,Norb,Nspin,Nbath,nup,ndw,ihf
  allocate(impHloc(Nlat,Nlat,Nspin,Nspin,Norb,Norb),Hbath(Nlat,Nlat,Nspin,Nspin,Norb,Norb,max(Nbath,1)),Vbath(Nlat,Nspin,Norb,max(Nbath,1)))
  read(u)impHloc
  if(Nbath>0)read(u)Hbath(:,:,:,:,:,:,1:Nbath)
  if(Nbath>0)read(u)Vbath(:,:,:,1:Nbath)
  read(u)Uloc,Ust,Jh,Jx,Jp,xmu
  close(u)
  if(Nlat*Norb/=nimp)stop "chi_check ERROR: written for two impurity orbitals"
  call gpu_build_Hv_sector(Nlat,Norb,Nspin,Nbath,nup,ndw,impHloc,Hbath(:,:,:,:,:,:,1:Nbath),Vbath(:,:,:,1:Nbath),Uloc,Ust,Jh,Jx,Jp,xmu,&
       ihf/=0,0,1)
  call gpu_sp_lanc_eigh_dev(e0,gs,512,threshold=1d-14)
  coef=0d0
  do a=1,nimp
     coef(a,1,a)=0.5d0; coef(a,2,a)=-0.5d0      !S^z_a
  enddo
  call gpu_apply_density_ops_dev(gs,coef,dv,mean,norm2)
  chi=(0d0,0d0)
  do b=1,nimp
     alanc=0d0; blanc=0d0; overlaps=(0d0,0d0); poles=0d0; weights=(0d0,0d0)
     call gpu_sp_lanc_tridiag_probes_dev(dv(b),dv,alanc,blanc,overlaps,nsteps=ns)
     call gpu_gf_from_probes(alanc(1:ns),blanc(1:ns),overlaps(:,1:ns),sqrt(norm2(b)),poles(1:ns),weights(:,1:ns))
     do k=1,nfreq
        z=cmplx(0d0,2d0*pi*ifreq(k)/beta,8)
        do n=1,ns
           de=poles(n)-e0
           if(abs(de)<=cutoff)cycle
           do a=1,nimp
              chi(k,a,b)=chi(k,a,b)-(weights(a,n)/(z-de)-conjg(weights(a,n))/(z+de))
           enddo
        enddo
     enddo
  enddo
  do a=1,nimp
     call gpu_free_vector(dv(a))
  enddo
  call gpu_free_vector(gs)
  call gpu_delete_Hv_sector()
  if(gpu_live_sectors()/=0)stop "chi_check ERROR: a sector is still open"
  write(*,"(A,ES24.16)")"E0= ",e0
  write(*,"(A,*(ES24.16))")"mean= ",mean
  write(*,"(A,*(ES24.16))")"norm2= ",norm2
  write(*,"(A,*(ES24.16))")"chi_re= ",dble(chi)
  write(*,"(A,*(ES24.16))")"chi_im= ",aimag(chi)
  write(*,"(A,I0)")"live_sectors= ",gpu_live_sectors()
end program chi_check
