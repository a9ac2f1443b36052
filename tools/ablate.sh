#!/bin/bash
# Builds measurement variants of the kernels (DMVAE_ABLATE=1..11: csrc/measure.h lists them) into
# deep-mixture-vae_amd/build/libdmvae_hip_abl<N>.so (git-ignored; select with DMVAE_HIP_LIB).
# Results of an ablated library are WRONG by construction: timing only.
set -e
cd "$(dirname "$0")/../deep-mixture-vae_amd"
python3 build.py > /dev/null
# the sources that read measure.h (the host side: step.hip the step without its gather, api.hip the stamp tables)
ABL="gemm_bf16 latent gemm_bf16_256 heads_dx heads_latent step api"
for n in "$@"; do
  for b in $ABL; do
    VF="-mllvm -amdgpu-mfma-vgpr-form=1"; if [ $b = latent ]; then VF=""; fi
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 $VF -I ../include -DDMVAE_ABLATE=$n -c csrc/$b.hip -o build/${b}_abl$n.o &
  done
done
wait
for n in "$@"; do
  objs=""
  for b in $(python3 -c "import build; print(' '.join(s[:-4] for s in build.SOURCES))"); do
    use=build/$b.o
    for a in $ABL; do if [ $a = $b ]; then use=build/${b}_abl$n.o; fi; done
    objs="$objs $use"
  done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o build/libdmvae_hip_abl$n.so $objs
  echo build/libdmvae_hip_abl$n.so
done
