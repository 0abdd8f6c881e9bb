"""CPU: the row widths the dense kernels are tested at (tests/test_gpu_row_widths.py), and the references at those widths.

Every dense kernel is parameterised by the row width.  The scans count it in k-tiles of 128 bytes per row: the fp16 copy
has KT = dim_pad / 64, the int8 copies KT = dim_pad8 / 128, with dim_pad = round_up(dim, 64) and dim_pad8 =
round_up(dim, 128) (hx_create).  What depends on the width: the ring parity of k_scan8's k-tile loop (odd KT), the resident
query tile of k_scan (KT <= QRES_KT = 6), the unrolled and the loop form of wave_spec_dot (dim_pad <= 1024 or not), the
element padding of k_prep_rows (dim % 64 != 0) and its zero fill of [dim_pad, dim_pad8).  WIDTHS names one width or more for
every such class; the first test fails when a width that is the only member of its class is dropped.  The second keeps the
GPU module's reference honest: the numpy oracle and its C restatement agree bit for bit at every width of the table."""
import os
import re

import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import oracle as O

QRES_KT = 6            # scan.hip: the query tile stays resident in LDS up to this many k-tiles (B <= 32)
SPEC_DOT_UNROLLED = 1024   # select.hip, wave_spec_dot: fully unrolled up to this dim_pad, a loop beyond

# dim -> (dim_pad, fp16 KT, dim_pad8, int8 KT), written out: the helper below has to reproduce it
WIDTH_TABLE = {
    65: (128, 2, 128, 1),        # 63 padding columns
    129: (192, 3, 256, 2),       # odd fp16 KT, padding in both copies
    192: (192, 3, 256, 2),       # odd fp16 KT, dim_pad != dim_pad8
    320: (320, 5, 384, 3),       # odd in both
    448: (448, 7, 512, 4),       # fp16 just past QRES_KT
    600: (640, 10, 640, 5),      # odd int8 KT, padding
    896: (896, 14, 896, 7),      # int8 just past QRES_KT, odd
    1000: (1024, 16, 1024, 8),   # last width of the unrolled wave_spec_dot, with padding
    1025: (1088, 17, 1152, 9),   # first width of its loop form, odd in both
    1536: (1536, 24, 1536, 12),  # common model width
    3072: (3072, 48, 3072, 24),  # common model width
}
WIDTHS = tuple(WIDTH_TABLE)
STAR_WIDTHS = (192, 320, 448, 896)     # the widths that pin a kernel path of the scans
OTHER_WIDTHS = (1, 63, 4096)           # the ends of the ABI's range: references only


def width_class(dim):
    """What the kernels see of a width, by hx_create's padding rules."""
    dim_pad = (dim + 63) // 64 * 64
    dim_pad8 = (dim + 127) // 128 * 128
    kt16, kt8 = dim_pad * 2 // 128, dim_pad8 // 128
    return dict(dim_pad=dim_pad, dim_pad8=dim_pad8, kt16=kt16, kt8=kt8,
                odd16=kt16 % 2 == 1, odd8=kt8 % 2 == 1,
                qres16=kt16 <= QRES_KT, qres8=kt8 <= QRES_KT,
                loop=dim_pad > SPEC_DOT_UNROLLED,
                elem_pad=dim % 64 != 0,
                pads_differ=dim_pad != dim_pad8)


# every class the width-dependent code paths distinguish: (key, value) has to occur in the table
CLASSES = [("odd16", True), ("odd16", False), ("odd8", True), ("odd8", False),
           ("qres16", True), ("qres16", False), ("qres8", True), ("qres8", False),
           ("loop", True), ("loop", False), ("elem_pad", True), ("elem_pad", False),
           ("pads_differ", True), ("pads_differ", False)]


def test_the_helper_reproduces_the_table():
    for dim, (dp, kt16, dp8, kt8) in WIDTH_TABLE.items():
        c = width_class(dim)
        assert (c["dim_pad"], c["kt16"], c["dim_pad8"], c["kt8"]) == (dp, kt16, dp8, kt8), dim
    assert set(STAR_WIDTHS) <= set(WIDTHS)


def test_the_constants_of_the_table_are_the_sources():
    """The classes are cut at constants of the HIP sources; a change there asks for another table."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rag_application_amd", "csrc")
    scan = open(os.path.join(csrc, "scan.hip")).read()
    m = re.search(r"constexpr\s+int\s+QRES_KT\s*=\s*(\d+)\s*;", scan)
    assert m and int(m.group(1)) == QRES_KT
    assert "a.row_bytes <= QRES_KT * 128" in scan
    select = open(os.path.join(csrc, "select.hip")).read()
    body = select[select.index("float wave_spec_dot("):]
    assert re.search(r"if\s*\(dim_pad\s*<=\s*%d\)" % SPEC_DOT_UNROLLED, body[:600])
    engine = open(os.path.join(csrc, "engine.hip")).read()
    assert "h->dim_pad = (int)round_up(dim, 64);" in engine and "h->dim_pad8 = (int)round_up(dim, 128);" in engine


def missing(widths, star):
    """The width classes no member of `widths` is in (`star`: the widths the multi-item scan tests run)."""
    cls = {d: width_class(d) for d in widths}
    out = [f"{k}={v}" for k, v in CLASSES if not [d for d in widths if cls[d][k] == v]]
    # both parities on both sides of QRES_KT for each copy: the three-stage ring of k_scan with odd and even KT,
    # with the resident and with the streamed query tile
    for odd, qres in ((True, True), (True, False), (False, True), (False, False)):
        for copy, o, q in (("fp16", "odd16", "qres16"), ("int8", "odd8", "qres8")):
            if not [d for d in widths if cls[d][o] == odd and cls[d][q] == qres]:
                out.append(f"{copy} odd={odd} qres={qres}")
    # odd KT > 1 for both copies, and the first KT past QRES_KT, among the widths the multi-item tests run
    for o, kt in (("odd16", "kt16"), ("odd8", "kt8")):
        if not [d for d in star if d in cls and cls[d][o] and cls[d][kt] > 1]:
            out.append(f"star {o}")
        if not [d for d in star if d in cls and cls[d][kt] == QRES_KT + 1]:
            out.append(f"star {kt}={QRES_KT + 1}")
    # element padding on both sides of wave_spec_dot's switch; the last unrolled and the first looped chunk count
    for loop in (True, False):
        if not [d for d in widths if cls[d]["loop"] == loop and cls[d]["elem_pad"]]:
            out.append(f"loop={loop} with element padding")
    if not [d for d in widths if cls[d]["dim_pad"] == SPEC_DOT_UNROLLED]:
        out.append("last unrolled width")
    if not [d for d in widths if cls[d]["dim_pad"] == SPEC_DOT_UNROLLED + 64]:
        out.append("first loop width")
    return out


def test_every_width_class_has_a_member():
    assert missing(WIDTHS, STAR_WIDTHS) == []


@pytest.mark.parametrize("dim", [448, 896, 1000, 1025])
def test_dropping_a_sole_member_is_noticed(dim):
    """The point of the class test, shown on the table itself: each of these widths is the only member of a class."""
    assert missing(tuple(d for d in WIDTHS if d != dim), tuple(d for d in STAR_WIDTHS if d != dim)) != []


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def same_lists(got, want, B, what):
    (s, i, c), (es, ei) = got, want
    for b in range(B):
        assert c[b] == len(ei[b]), (what, b)
        np.testing.assert_array_equal(i[b, :c[b]], ei[b], err_msg=f"{what} b={b}: ids")
        np.testing.assert_array_equal(bits(s[b, :c[b]]), bits(es[b]), err_msg=f"{what} b={b}: score bits")


@pytest.mark.parametrize("dim", WIDTHS + OTHER_WIDTHS)
def test_numpy_and_c_oracle_agree_at_every_width(dim):
    """cosine_preprocess, dense top-L, prefix top-L, quantize_i8 and search_i8 on unit rows: ids and fp32 bits."""
    n, B, L = 700, 5, 20
    X = O.synth_dense(31, 0, n, dim) * np.float32(2.5)
    Q = O.synth_dense(32, 0, B, dim) * np.float32(0.3)
    np.testing.assert_array_equal(bits(CO.synth_dense(31, 0, n, dim) * np.float32(2.5)), bits(X))
    Xn, Qn = O.cosine_preprocess(X), O.cosine_preprocess(Q)
    np.testing.assert_array_equal(bits(CO.cosine_preprocess(X)), bits(Xn))
    np.testing.assert_array_equal(bits(CO.cosine_preprocess(Q)), bits(Qn))
    ids = np.arange(n)
    want = list(zip(*[O.topk(O.spec_dot(Xn, Qn[b]), ids, L) for b in range(B)]))
    same_lists(CO.search_dense(Xn, Qn, L), want, B, f"dense dim={dim}")
    for m in (64, 192, 320):
        if m > dim:
            continue
        Xm, Qm = O.cosine_preprocess(X[:, :m]), O.cosine_preprocess(Q[:, :m])
        np.testing.assert_array_equal(bits(CO.cosine_preprocess(X, m)), bits(Xm))
        np.testing.assert_array_equal(bits(CO.cosine_preprocess(Q, m)), bits(Qm))
        want = list(zip(*[O.topk(O.spec_dot(Xm, Qm[b]), ids, L) for b in range(B)]))
        same_lists(CO.search_dense(Xm, Qm, L), want, B, f"prefix {m} dim={dim}")
    X8, rx = CO.quantize_i8(Xn)
    Q8, rq = CO.quantize_i8(Qn)
    np.testing.assert_array_equal(X8, O.quantize_i8(Xn))
    np.testing.assert_array_equal(Q8, O.quantize_i8(Qn))
    np.testing.assert_array_equal(bits(rx), bits(O.i8_norm_inv(X8)))
    np.testing.assert_array_equal(bits(rq), bits(O.i8_norm_inv(Q8)))
    want = list(zip(*[O.topk(O.i8_scores(X8, Q8[b]), ids, L) for b in range(B)]))
    same_lists(CO.search_i8(X8, rx, Q8, rq, L), want, B, f"i8 dim={dim}")
