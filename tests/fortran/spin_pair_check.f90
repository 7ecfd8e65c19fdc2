!> Test host for tests/test_gpu_fortran_spin_pair.py: reads a model and the ground state's sector (nup,ndw) from the raw file named on the
!! command line (stream I/O, written by the test, the format of chi_check.f90), finds the ground state on the device (gpu_sp_lanc_eigh_dev),
!! keeps its sector, and computes the local pair susceptibility chi_ab(i nu_n), O_a = c_{a,up} c_{a,dw} on the two impurity sites, n = 0, 1,
!! 5 at beta = 50: O_a|gs> in the sector (nup-1,ndw-1) and O_a^+|gs> in (nup+1,ndw+1) by gpu_apply_spin_pair_dev, one
!! gpu_sp_lanc_tridiag_probes_dev run per operator and sector, gpu_gf_from_probes.  Prints E0, the norms and chi; frees everything and stops
!! unless no sector is left open.
program spin_pair_check
  use ED_HAMILTONIAN_GPU_HXV
  implicit none
  integer,parameter          :: nlanc=400,nimp=2,nfreq=3
  real(8),parameter          :: beta=50d0,pi=3.141592653589793238d0
  integer,parameter          :: ifreq(nfreq)=[0,1,5]
  integer(4)                 :: Nlat,Norb,Nspin,Nbath,nup,ndw,ihf
  complex(8),allocatable     :: impHloc(:,:,:,:,:,:),Hbath(:,:,:,:,:,:,:)
  real(8),allocatable        :: Vbath(:,:,:,:)
  real(8)                    :: Uloc(5),Ust,Jh,Jx,Jp,xmu,e0,alanc(nlanc),blanc(nlanc),poles(nlanc),norm2(nimp,2),de
  complex(8)                 :: overlaps(nimp,nlanc),weights(nimp,nlanc),chi(nfreq,nimp,nimp),z
  type(gpu_vector)           :: gs,dv(nimp)
  character(len=512)         :: path
  integer                    :: u,ns,a,b,n,k,side,d
  logical                    :: create
  call get_command_argument(1,path)
  open(newunit=u,file=trim(path),access="stream",form="unformatted",status="old")
  read(u)Nlat,Norb,Nspin,Nbath,nup,ndw,ihf
  allocate(impHloc(Nlat,Nlat,Nspin,Nspin,Norb,Norb),Hbath(Nlat,Nlat,Nspin,Nspin,Norb,Norb,max(Nbath,1)),Vbath(Nlat,Nspin,Norb,max(Nbath,1)))
  read(u)impHloc
  if(Nbath>0)read(u)Hbath(:,:,:,:,:,:,1:Nbath)
  if(Nbath>0)read(u)Vbath(:,:,:,1:Nbath)
  read(u)Uloc,Ust,Jh,Jx,Jp,xmu
  close(u)
  if(Nlat*Norb/=nimp)stop "spin_pair_check ERROR: written for two impurity orbitals"
  call gpu_build_Hv_sector(Nlat,Norb,Nspin,Nbath,nup,ndw,impHloc,Hbath(:,:,:,:,:,:,1:Nbath),Vbath(:,:,:,1:Nbath),Uloc,Ust,Jh,Jx,Jp,xmu,&
       ihf/=0,0,1)
  call gpu_sp_lanc_eigh_dev(e0,gs,512,threshold=1d-14)
  call gpu_keep_sector(gs)
  chi=(0d0,0d0)
  do side=1,2                                    !1: O^+|gs> in (nup+1,ndw+1), poles at z = +de;  2: O|gs> in (nup-1,ndw-1), poles at z = -de
     create=side==1
     d=merge(1,-1,create)
     call gpu_build_Hv_sector(Nlat,Norb,Nspin,Nbath,nup+d,ndw+d,impHloc,Hbath(:,:,:,:,:,:,1:Nbath),Vbath(:,:,:,1:Nbath),Uloc,Ust,Jh,Jx,Jp,xmu,&
          ihf/=0,0,1)
     do a=1,nimp
        call gpu_apply_spin_pair_dev(gs,[a],[a],[(1d0,0d0)],create,create,dv(a),norm2(a,side))
     enddo
     do b=1,nimp
        alanc=0d0; blanc=0d0; overlaps=(0d0,0d0); poles=0d0; weights=(0d0,0d0)
        call gpu_sp_lanc_tridiag_probes_dev(dv(b),dv,alanc,blanc,overlaps,nsteps=ns)
        call gpu_gf_from_probes(alanc(1:ns),blanc(1:ns),overlaps(:,1:ns),sqrt(norm2(b,side)),poles(1:ns),weights(:,1:ns))
        do k=1,nfreq
           z=cmplx(0d0,2d0*pi*ifreq(k)/beta,8)
           do n=1,ns
              de=poles(n)-e0
              do a=1,nimp
                 if(side==1)then
                    chi(k,a,b)=chi(k,a,b)-weights(a,n)/(z-de)       !<O_a^+ gs|n><n|O_b^+ gs>
                 else
                    chi(k,b,a)=chi(k,b,a)+weights(a,n)/(z+de)       !run from O_b gs, probe O_a gs: row b of the second sum
                 endif
              enddo
           enddo
        enddo
     enddo
     do a=1,nimp
        call gpu_free_vector(dv(a))
     enddo
     call gpu_delete_Hv_sector()
  enddo
  call gpu_free_vector(gs)
  if(gpu_live_sectors()/=0)stop "spin_pair_check ERROR: a sector is still open"
  write(*,"(A,ES24.16)")"E0= ",e0
  write(*,"(A,*(ES24.16))")"norm2= ",norm2
  write(*,"(A,*(ES24.16))")"chi_re= ",dble(chi)
  write(*,"(A,*(ES24.16))")"chi_im= ",aimag(chi)
  write(*,"(A,I0)")"live_sectors= ",gpu_live_sectors()
end program spin_pair_check
