"""Diagnostic: L and M segment lengths of k_scan8q by phase position (needs the -DHX_S8Q_STAMP library built in-tree:
python -c "from rag_application_amd import build; build.build(defines=('HX_S8Q_STAMP',), lib='rag_application_amd/csrc/build/libhx_s8q_stamp.so', objdir='rag_application_amd/csrc/build/s8q_stamp')")
Usage: python scripts/s8q_stamps.py [rows [batch]]   (dense int8-candidate searches only; s_memtime = shader cycles; the
stamps themselves lengthen every segment, so the table compares two builds that carry the same stamps, not a timed run)"""
import os, sys, ctypes, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["HX_LIB_PATH"] = os.path.abspath("rag_application_amd/csrc/build/libhx_s8q_stamp.so")
import torch
from rag_application_amd import engine as eng, synth, _lib
N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
NS = 16
assert eng.scan8_form(B, 768, "i8") == 3, "this batch does not take k_scan8q"
ix = eng.HxIndex(768, ())
ix.reserve(N); ix.synth_fill(N, synth.SEED_CORPUS)
ix.set_dense_candidates("i8")
q = eng.synth_queries_dense(768, 0, B, synth.SEED_QUERY)
fn = _lib.lib().hx_debug_s8q_stamps
fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
def read():
    buf = np.zeros(256 * 2 * NS, np.uint64)
    assert fn(buf.ctypes.data, buf.size) == 0
    return buf.reshape(256, 2, NS).astype(np.float64)
for _ in range(3): ix.search_dense(q, 100)
torch.cuda.synchronize()
REPS = 5
s0 = read()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
ev[0].record()
for _ in range(REPS): ix.search_dense(q, 100)
ev[1].record(); torch.cuda.synchronize()
st = read() - s0
print("search_dense ms %.3f (stamped build)  rows %d  B %d" % (ev[0].elapsed_time(ev[1]) / REPS, N, B))
items = st[:, :, 13]
live = items[:, 0] > 0
print("workgroups with items %d of 256; items per workgroup and search: mean %.1f max %.0f" % (live.sum(), items[live, 0].mean() / REPS, items[:, 0].max() / REPS))
names = ["L segment", "wait at its barrier", "M segment", "wait at its barrier"]
for g in (0, 1):
    s, n = st[live, g, :], items[live, g][:, None]
    per = s[:, :12] / n
    print("group %d (wave %d): cycles per item %.0f" % (g, 4 * g, per.sum(1).mean()))
    for pos, pn in enumerate(("first phase", "middle phases", "last phase")):
        row = "  ".join("%s %7.1f" % (names[i], per[:, pos * 4 + i].mean()) for i in range(4))
        print("  %-13s %s   sum %7.1f" % (pn, row, per[:, pos * 4:pos * 4 + 4].sum(1).mean()))
    print("  deferred filter inside the first L segment (decision + log stores): %.1f cycles per item" % (s[:, 12] / n[:, 0]).mean())
