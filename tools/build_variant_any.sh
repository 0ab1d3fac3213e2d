#!/bin/bash
# developer tool: experimental libukm_exp_TAG.so with extra -D flags for ONE source file
# usage: build_variant_any.sh <setops|sort|encode|scan|nway|kway|tax|ctx|srmerge|probe_union|...> TAG [-DFOO=1 ...]
# (the other objects are those of the last `python -m unikmer_amd.build`; the list of sources is build.py's)
set -e
R=$(cd "$(dirname "$0")/.." && pwd); C=$R/unikmer_amd/csrc; which=$1; tag=$2; shift 2
srcs=$(cd "$R" && python3 -c "from unikmer_amd.build import SOURCES; print(' '.join(s[len('ukm_'):-len('.hip')] for s in SOURCES))")
case " $srcs " in *" $which "*) ;; *) echo "no source ukm_$which.hip in build.py's SOURCES: $srcs" >&2; exit 1;; esac
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC "$@" -c $C/ukm_$which.hip -o /tmp/var_${which}_$tag.o
objs=""
for f in $srcs; do
  if [ $f = $which ]; then objs="$objs /tmp/var_${which}_$tag.o"; else objs="$objs $C/ukm_$f.o"; fi
done
hipcc --offload-arch=gfx950 -shared -fPIC -o $R/unikmer_amd/libukm_exp_$tag.so $objs
echo built $tag
