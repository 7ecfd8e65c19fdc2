!> Test host for tests/test_gpu_fortran_one_body.py: reads a model and the ground state's sector (nup,ndw) from the raw file named on the
!! command line (stream I/O, written by the test, the format of spin_pair_check.f90), finds the ground state on the device
!! (gpu_sp_lanc_eigh_dev) and computes, inside that sector, the bond and current operators of the orbital pair (1,2),
!!     B = sum_s (c^+_1s c_2s + h.c.),   J = i sum_s (c^+_1s c_2s - h.c.),
!! by gpu_apply_one_body_dev: their means, the norms of the fluctuations, the mean of the single hop c^+_1,up c_2,up without subtraction, and
!! the susceptibility chi_ab(i nu_n), n = 0, 1, 5 at beta = 50, from one gpu_sp_lanc_tridiag_probes_dev run per operator and
!! gpu_gf_from_probes (both operators are Hermitian: one run set, poles within 1d-8 of the state left out).  Prints E0, the means, the
!! norms and chi; frees everything and stops unless no sector is left open.
program one_body_check
  use ED_HAMILTONIAN_GPU_HXV
  implicit none
  integer,parameter          :: nlanc=36,nops=2,nfreq=3       !nlanc = Dim of the 2x2 plaquette's sector (2,2), which the test sends
  real(8),parameter          :: beta=50d0,pi=3.141592653589793238d0
  integer,parameter          :: ifreq(nfreq)=[0,1,5]
  integer(4)                 :: Nlat,Norb,Nspin,Nbath,nup,ndw,ihf
  complex(8),allocatable     :: impHloc(:,:,:,:,:,:),Hbath(:,:,:,:,:,:,:)
  real(8),allocatable        :: Vbath(:,:,:,:)
  real(8)                    :: Uloc(5),Ust,Jh,Jx,Jp,xmu,e0,alanc(nlanc),blanc(nlanc),poles(nlanc),norm2(nops),hop_norm2,de
  complex(8)                 :: overlaps(nops,nlanc),weights(nops,nlanc),chi(nfreq,nops,nops),z,mean(nops),hop_mean
  type(gpu_vector)           :: gs,dv(nops),hop
  character(len=512)         :: path
  integer                    :: u,ns,a,b,n,k
  complex(8),parameter       :: one=(1d0,0d0),xi=(0d0,1d0)
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
  !(spin, to, from, coef), 1-based: up 1<-2, up 2<-1, dw 1<-2, dw 2<-1
  call gpu_apply_one_body_dev(gs,[1,1,2,2],[1,2,1,2],[2,1,2,1],[one,one,one,one],dv(1),mean(1),norm2(1))
  call gpu_apply_one_body_dev(gs,[1,1,2,2],[1,2,1,2],[2,1,2,1],[xi,-xi,xi,-xi],dv(2),mean(2),norm2(2))
  call gpu_apply_one_body_dev(gs,[1],[1],[2],[one],hop,hop_mean,hop_norm2,subtract_mean=.false.)
  chi=(0d0,0d0)
  do b=1,nops
     alanc=0d0; blanc=0d0; overlaps=(0d0,0d0); poles=0d0; weights=(0d0,0d0)
     call gpu_sp_lanc_tridiag_probes_dev(dv(b),dv,alanc,blanc,overlaps,nsteps=ns)
     call gpu_gf_from_probes(alanc(1:ns),blanc(1:ns),overlaps(:,1:ns),sqrt(norm2(b)),poles(1:ns),weights(:,1:ns))
     do k=1,nfreq
        z=cmplx(0d0,2d0*pi*ifreq(k)/beta,8)
        do n=1,ns
           de=poles(n)-e0
           if(abs(de)<=1d-8)cycle
           do a=1,nops
              chi(k,a,b)=chi(k,a,b)-(weights(a,n)/(z-de)-conjg(weights(a,n))/(z+de))
           enddo
        enddo
     enddo
  enddo
  do a=1,nops
     call gpu_free_vector(dv(a))
  enddo
  call gpu_free_vector(hop)
  call gpu_free_vector(gs)
  call gpu_delete_Hv_sector()
  if(gpu_live_sectors()/=0)stop "one_body_check ERROR: a sector is still open"
  write(*,"(A,ES24.16)")"E0= ",e0
  write(*,"(A,*(ES24.16))")"mean_re= ",dble(mean)
  write(*,"(A,*(ES24.16))")"mean_im= ",aimag(mean)
  write(*,"(A,*(ES24.16))")"norm2= ",norm2
  write(*,"(A,*(ES24.16))")"hop= ",dble(hop_mean),aimag(hop_mean),hop_norm2
  write(*,"(A,*(ES24.16))")"chi_re= ",dble(chi)
  write(*,"(A,*(ES24.16))")"chi_im= ",aimag(chi)
  write(*,"(A,I0)")"live_sectors= ",gpu_live_sectors()
end program one_body_check
