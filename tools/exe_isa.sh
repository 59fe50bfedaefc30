#!/bin/bash
# Static account of the stream roles' out-of-line functions (32-slot window build, worker state
# in LDS) in the current sources, from the compiler's own assembly: code bytes, instructions,
# branches, s_nop, s_waitcnt, lane moves, scratch accesses, and the lane moves to and from each
# VGPR the prologue saves with all lanes on: those hold SGPRs (the callee-saved ones, written
# once in the prologue and read once in the epilogue, and the register allocator's SGPR spills).
# Ordinary instructions only.
# usage: tools/exe_isa.sh [-i OLD.s | -o KEEP.s] [extra -D flags]   (no GPU needed)
cd "$(dirname "$0")/.."
TMP=$(mktemp -d)
ASM=$TMP/dev.s
BUILD=1
if [ "$1" = "-o" ]; then ASM=$2; shift 2; elif [ "$1" = "-i" ]; then ASM=$2; BUILD=0; shift 2; fi
if [ $BUILD = 1 ]; then
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fPIC \
    -mllvm -amdgpu-lower-module-lds-strategy=module --cuda-device-only -S "$@" -o "$ASM" distributed_amd/csrc/dgplace.hip 2>/dev/null || exit 1
fi
echo "# bytes insts branches(unconditional) s_nop s_waitcnt writelane readlane scratch function [sgpr-holding vgpr:writes/reads ...]"
for f in $(grep -o -E "^_ZN3dgp2st[0-9]+([A-Za-z_0-9]*ILb1E|[a-z_]*(_cold|_each)E)[A-Za-z_0-9]*:" "$ASM" | tr -d ':'); do
  awk -v f="$f" '
    $0 ~ "^" f ":" {on = 1; next}
    on && /^\.Lfunc_end/ {on = 2; next}
    on == 1 && /^\t[a-z]/ {
      n++
      if ($1 ~ /^s_(c?branch|setpc|swappc|call)/) {br++; if ($1 == "s_branch") ub++}
      if ($1 == "s_nop") nop++
      if ($1 == "s_waitcnt") wc++
      if (n < 8 && $1 ~ /^s_(or|xor)_saveexec/) wwm = 1
      if (wwm && $1 == "s_mov_b64" && $2 == "exec,") wwm = 0
      if (wwm && $1 == "scratch_store_dword") {v = $3; sub(",", "", v); hold[v] = 1}
      if ($1 ~ /^v_writelane/) {wl++; v = $2; sub(",", "", v); if (v in hold) hw[v]++}
      if ($1 ~ /^v_readlane/) {rl++; v = $3; sub(",", "", v); if (v in hold) hr[v]++}
      if ($1 ~ /^scratch_/) sc++
    }
    on == 2 && /codeLenInByte/ {bytes = $NF; on = 0}
    END {printf "%d %d %d(%d) %d %d %d %d %d %s", bytes, n, br, ub, nop, wc, wl, rl, sc, f
         for (v in hold) printf " %s:%d/%d", v, hw[v], hr[v]
         printf "\n"}' "$ASM"
done > $TMP/acct.txt
c++filt < $TMP/acct.txt | sed -e 's/dgp::st:://' -e 's/void //'
awk '{t += $1} END {print "# sum of the listed functions:", t, "bytes"}' $TMP/acct.txt
rm -rf $TMP
