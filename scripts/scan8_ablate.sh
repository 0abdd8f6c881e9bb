# ablations of the int8 candidate scan (timing builds, wrong results): HX_SCAN_DBG = 1 one corpus tile over and over (no HBM
# traffic), 2 no loads in the loop, 3 no MFMAs, 4 no threshold filter,
# 5 no fragment reads in the loop, 6 MFMAs + barriers only, 7 MFMAs only, 8 no loads and no filter; 12 the query-stationary
# form (k_scan8q) without its global_load_lds, 13 the same form without its filter.  0 is the shipped routing (k_scan8q at this shape); every other value times
# k_scan8, as does "old" (HX_DEBUG_NO_QS).  The library: python -c "from rag_application_amd import build as b; b.build(
# defines=('HX_SCAN_DBG',), lib='scripts/ubench/build/libhx_dbg.so', objdir='scripts/ubench/build/obj_dbg')".
# usage (GPU box): bash scripts/scan8_ablate.sh
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
export HX_LIB_PATH=$R/scripts/ubench/build/libhx_dbg.so AB_L=100
for D in ${ABLATE:-0 12 13 old 4 1 2 8 5 6 7 3}; do
  echo "== HX_SCAN_DBG=$D"
  if [ $D = old ]; then export HX_DEBUG_NO_QS=1; D=0; else unset HX_DEBUG_NO_QS; fi
  HX_SCAN_DBG=$D timeout -k 10 120 python $R/scripts/cand8_hits.py 2>&1 | grep -E "^\{" | cut -c1-300 || { echo "HX_SCAN_DBG=$D failed: stopping"; exit 1; }
done
