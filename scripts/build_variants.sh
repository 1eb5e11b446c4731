#!/bin/bash
# Build diagnostic variants of libns_hip.so HERE (cross-compile) so GPU-box minutes are not spent compiling:
#   scripts/build_variants.sh name1:"-DFLAG=1" name2:"-DFLAG=2" ...   ->  variants/libns_hip_<name>.so
set -e
cd "$(dirname "$0")/../neural-speed_amd/csrc"
mkdir -p ../../variants
all_objs=$(make -s objs)  # the library's object list, in link order
for spec in "$@"; do
  name=${spec%%:*}; flags=${spec#*:}
  # FILES = which kernel sources get the flags (the others are linked from the regular build); ns_gemv = gemv_kernel's slice objects
  # (ns_gemv_<KIND>_<SPS>.o, defines as in the Makefile) and its host file
  objs=""
  for o in $all_objs; do
    b=${o%.o}; f=$b; src="$b.hip"
    case $b in
      ns_gemv_host|ns_gemv_plan) f=ns_gemv; src="-x hip $b.cpp" ;;  # (the host files see the kernels' parameter structs: same flags)
      ns_gemvs_k) f=ns_gemvs; src="ns_gemvs.hip" ;;                  # FILES=ns_gemvs: gemvs_kernel ...
      ns_gemvs|ns_gemvs_plan) f=ns_gemvs; src="-x hip $b.cpp" ;;     # ... and its host files
      ns_attn_decode|ns_attn_prefill) f=ns_attn ;;  # FILES=ns_attn: the attention kernels (ablation builds: NS_AS_ABL, NS_A2_ABL, NS_ATTN_U ...)
      ns_attn|ns_attn_plan) f=host ;;               # ... not their host code (.cpp, linked from the regular build)
      ns_gemm2|ns_gemm3) f=ns_gemm ;;               # FILES=ns_gemm: the two prefill GEMM kernel files
      ns_gemm|ns_gemm_plan|ns_scratch) f=host ;;    # ... not their host code
      ns_route|ns_route_fuse|ns_route_exec) f=host ;;  # the device route: host code
      ns_gemv_*_*) f=ns_gemv; IFS=_ read -r _ _ kind sps <<<"$b"; src="-DNS_GEMV_KIND=$kind -DNS_GEMV_SPS=$sps ns_gemv.hip" ;;
    esac
    if [[ " ${FILES:-ns_kernels ns_gemv ns_gemm} " == *" $f "* ]]; then
      while (( $(jobs -rp | wc -l) >= ${JOBS:-8} )); do wait -n; done
      /opt/rocm/bin/hipcc -O3 -std=c++20 $flags -fPIC --offload-arch=gfx950 -c $src -o /tmp/${b}_$name.o &
      objs="$objs /tmp/${b}_$name.o"
    else
      objs="$objs $o"
    fi
  done
  wait
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../variants/libns_hip_$name.so $objs -ldl
  echo built variants/libns_hip_$name.so
done
