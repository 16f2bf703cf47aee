"""Cases and wrong loaders of the K5 (s2m2_conv2d, csrc/conv.hip) patch-kernel tests: the v3 halo tiles (tile ids 12, 13, 19, 23, 24, 25, 26 and
what the heuristic picks, K order 0, fp16 and fp32) and the v5 fragment-stream kernel (K order 2, fp16; 2x32, 4x32 and 4x40 pixel patches, blocks
of 128 or 192 output channels).  Shared by tests/test_hip_k5_patch.py (the kernels) and tests/test_k5_patch_cases_cpu.py (the construction
without them).  The float64 reference, bound(), compare(), wide(), ulp() and the table helpers are those of tests/k5_cases.py, used as they are;
that module's docstring describes operands, regimes, the bound and the comparator.  Only what the patch kernels add is here.

What is under test: a block owns a patch of PH x PW output pixels and loads the patch plus its halo ((PH + KH - 1) x (PW + KW - 1) pixels)
once per channel chunk (CH channels: 64 bytes ... 128 bytes per pixel on the halo tiles, 128 or 192 channels on the fragment stream), a halo
pixel outside the image coming from a block of zeros; a chunk is made of 16-byte pieces, each of which picks its source; pieces past Cin in
the last chunk come from the zero block too; the K loop runs (chunk, tap); grid.y walks blocks of BN output channels; on 4x40 patches the
MFMA tiles of 32 pixels run across patch rows (pixel q of the patch is (q / 40, q % 40)); a patch pixel outside the image is not stored.

Layers (LAYERS)   all stride 1, splits [(c, c) ...]:  3x3 128 -> 128 (ConvBlock2D) and 256 -> 256 (two chunks of 128, two cout blocks of 128, four
                  of 64);  3x1 / 1x3 [128, 128] -> 128 (the GRU passes);  1x3 [128, 128] -> 256 with SIGMOID, EPI_MUL and epi_cout0 = 128 (K17's
                  stacked z | r layer);  3x3 [96, 64, 32] -> 384 (Cin = 192 on chunks of 128: source boundaries inside a chunk, a half-empty
                  last chunk);  3x3 [128, 128, 64, 64] -> 128 (three chunks, all four source slots);  3x3 192 -> 192 and 1x3 [192, 192] -> 192
                  (blocks of 192 couts on chunks of 192, six waves);  3x3 [96, 96] -> 576 (three blocks of 192, a source boundary inside the
                  chunk);  halo tiles only: 3x3 [8, 128] -> 136 (Cin tail inside a chunk, Cout tail in the last block), 3x3 24 -> 64 (less
                  than one chunk), 3x3 128 -> 8 (a narrow head).  frag_layers() -- pack.frag_eligible() -- says which run on the fragment stream.
Shapes (SHAPES)   (1,1,1) (1,1,45) (1,9,1): one row, one column, most of the halo outside;  (1,2,32) (1,4,32) (1,4,40): exactly one patch of each
                  form;  (1,3,31) (1,3,39): one pixel short on both axes;  (1,5,33) (1,5,41): one pixel over, the halo crosses a patch seam and all
                  four image borders;  (2,8,64) (2,8,80): exact tilings of 32 and of 40;  (3,9,70): several patches, ragged, the middle image has
                  a neighbour above and below.  All on 3x3_128; (1,5,41), (3,9,70) and a single-patch shape on every other layer.
Regimes           `exact` (NONE, RELU; sum |w| |x| + |b| <= 2048, asserted by build_case()) and `gauss` (NONE, RELU, GELU, SIGMOID, TANH; out_scale
                  1 and 0.5; ADD, MUL, GRU, GATEMIX), as in k5_cases.  Every layer meets `exact` on (3,9,70); GRU and GATEMIX sit on the 3x1 and
                  1x3 layers, where the forward uses them.
Launches          Spec.halo: the halo tile ids (0 = the heuristic) the case runs on in both dtypes;  Spec.frag: the `tile=` values (2, 4, 40 for the
                  2x32, 4x32, 4x40 patch, 0 for conv_select_frag's own choice) it runs on in fp16.  conv_select_frag refuses a two-operand
                  epilogue on tile 4 and 40: launches() leaves those out by rule (REFUSED; the GPU test asserts the refusals); a launch with
                  epi_cout0 exists in K order 2 only.  selection() runs every launch through csrc/conv_select.h on the host (the program of
                  tests/test_select_cpu.py): chosen() is the kernel that runs, forced() the one a forced tile must give; the tests assert
                  that they agree and the table prints chosen().
Wrong loaders     wrong(case, variant, PH, PW, CH, BN): the layer by an explicit gather the way these kernels address it -- patch origin, pixel q of
                  the patch, halo pixel (hy, hx), input pixel or the zero block, a chunk of 16-byte pieces each with its source, (chunk, tap)
                  weights, cout blocks of BN -- with every source read from the flat NaN-surrounded buffer of wide().  VARIANTS, one defect each:
                    image_wrap, row_wrap     a halo pixel above / below (left / right of) the image is read at its flat index
                    pad_less                 padding K // 2 - 1
                    stride_of_src0           sources 1 .. 3 addressed with the pixel stride of source 0
                    seam_zero                a halo pixel that belongs to the neighbouring patch is read as zero
                    chunk_tail_reads_on      the pieces past Cin of a partly filled last chunk are read from memory (NaN from wide()'s padding)
                    src_boundary_at_chunk    the source is chosen per chunk, by the chunk's first channel, not per piece
                    raster_32                on a 4x40 patch pixel q reads its operand at (q / 32, q % 32); past the halo tile: zero
                    chunk_tap_swapped        the weights are consumed in (tap, chunk) order
                    cout_block_stride        cout block y uses the weights and the bias of block 0
                    epi_cout0_ignored        the epilogue is applied to every cout block (its operand indexed with the cout, as the kernel does)
                    partial_patch_stored     a patch pixel outside the image is stored to the address its raster index gives
                  differs() says, by construction, on which (case, form) a variant computes something else.
"""
import collections
import functools

import torch

import k5_cases as K
from k5_cases import (ACT_GELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, EPI_ADD, EPI_GATEMIX, EPI_GRU, EPI_MUL, EPI_NONE,   # noqa: F401
                      Layer, bound, compare, line, ulp, wide)
from s2m2_amd import pack

HALO = (0, 12, 13, 19, 23, 24, 25, 26)                  # 0 and every id conv_select.h maps to the halo family
FRAG = (2, 4, 40, 0)                                    # tile= of a K order 2 launch: the patch forms 2x32, 4x32, 4x40 and the selector's choice
FRAG_PATCH = {2: (2, 32), 4: (4, 32), 40: (4, 40)}
HALO_BN = {12: 128, 13: 64, 19: 128, 23: 64, 24: 64, 25: 64, 26: 128}    # conv_select.h
HALO_CH = {"float16": 64, "float32": 32}                # 128 bytes of channels
REFUSED = tuple((e, t) for e in (EPI_GRU, EPI_GATEMIX) for t in (4, 40))   # conv_select_frag: 128- and 160-pixel blocks take one operand

LAYERS = {
    "3x3_128": Layer(3, 3, 1, (128,), 128),
    "3x3_256": Layer(3, 3, 1, (256,), 256),
    "3x1_128+128": Layer(3, 1, 1, (128, 128), 128),
    "1x3_128+128": Layer(1, 3, 1, (128, 128), 128),
    "1x3_zr": Layer(1, 3, 1, (128, 128), 256),
    "3x3_96+64+32_384": Layer(3, 3, 1, (96, 64, 32), 384),
    "3x3_128+128+64+64": Layer(3, 3, 1, (128, 128, 64, 64), 128),
    "3x3_192": Layer(3, 3, 1, (192,), 192),
    "1x3_192+192": Layer(1, 3, 1, (192, 192), 192),
    "3x3_96+96_576": Layer(3, 3, 1, (96, 96), 576),
    "3x3_8+128_136": Layer(3, 3, 1, (8, 128), 136),
    "3x3_24_64": Layer(3, 3, 1, (24,), 64),
    "3x3_128_8": Layer(3, 3, 1, (128,), 8),
}
SHAPES = ((1, 1, 1), (1, 1, 45), (1, 9, 1), (1, 2, 32), (1, 4, 32), (1, 4, 40), (1, 3, 31), (1, 3, 39), (1, 5, 33), (1, 5, 41), (2, 8, 64), (2, 8, 80),
          (3, 9, 70))
ONE_PATCH = ((1, 2, 32), (1, 4, 32), (1, 4, 40))
OVER, RAGGED = (1, 5, 41), (3, 9, 70)

Spec = collections.namedtuple("Spec", "layer shape regime act scale epi epi_cout0 halo frag")


def frag_chunk(L):
    return pack.frag_chunk(pack.pad8(L.Cout), sum(L.cs))


def frag_layers():
    """the layers the fragment-stream kernel takes"""
    return tuple(n for n, L in LAYERS.items() if pack.frag_eligible(pack.pad8(L.Cout), sum(L.cs), L.KH, L.KW, torch.float16))


def _specs():
    s = {}
    eligible = frag_layers()

    def add(layer, shape, regime, act=ACT_NONE, scale=1.0, epi=EPI_NONE, epi_cout0=0):
        name = f"{layer}-{'x'.join(map(str, shape))}-{regime}"
        if regime == "gauss":
            name += f"-{K.ACT_NAME[act]}" + (f"-x{scale:g}" if scale != 1.0 else "") + (f"-{K.EPI_NAME[epi]}" if epi else "")
        elif act:
            name += f"-{K.ACT_NAME[act]}"
        assert name not in s, name
        halo = () if epi_cout0 else HALO                                  # epi_cout0 exists in K order 2 only
        frag = tuple(t for t in FRAG if (epi, t) not in REFUSED) if layer in eligible else ()
        s[name] = Spec(layer, shape, regime, act, scale, epi, epi_cout0, halo, frag)

    for i, shape in enumerate(SHAPES):                                  # every shape on ConvBlock2D's layer
        add("3x3_128", shape, "exact", ACT_RELU if i % 2 else ACT_NONE)
    add("3x3_128", (1, 1, 45), "gauss", ACT_TANH)
    add("3x3_128", (1, 4, 40), "gauss", ACT_RELU)
    add("3x3_128", (1, 3, 31), "gauss", ACT_SIGMOID, 0.5)
    add("3x3_128", (1, 5, 33), "gauss", ACT_TANH, 0.5)
    add("3x3_128", OVER, "gauss", ACT_GELU)
    add("3x3_128", OVER, "gauss", ACT_RELU, 1.0, EPI_MUL)
    add("3x3_128", (2, 8, 80), "gauss", ACT_SIGMOID)
    add("3x3_128", (2, 8, 64), "gauss", ACT_GELU, 0.5, EPI_ADD)
    add("3x3_128", RAGGED, "gauss", ACT_NONE, 0.5)
    add("3x3_128", RAGGED, "gauss", ACT_NONE, 1.0, EPI_ADD)
    add("3x3_256", (1, 2, 32), "exact", ACT_RELU)
    add("3x3_256", RAGGED, "exact")
    add("3x3_256", OVER, "gauss", ACT_GELU)
    add("3x3_256", RAGGED, "gauss", ACT_NONE, 1.0, EPI_ADD)
    for layer, one in (("3x1_128+128", (1, 4, 32)), ("1x3_128+128", (1, 4, 40))):      # the GRU passes
        add(layer, one, "exact", ACT_RELU)
        add(layer, RAGGED, "exact")
        add(layer, OVER, "gauss", ACT_TANH, 1.0, EPI_GRU)
        add(layer, RAGGED, "gauss", ACT_TANH, 1.0, EPI_GRU)
        add(layer, OVER, "gauss", ACT_SIGMOID, 1.0, EPI_GATEMIX)
        add(layer, RAGGED, "gauss", ACT_NONE, 0.5, EPI_GATEMIX)
    add("1x3_zr", RAGGED, "exact")
    add("1x3_zr", (1, 4, 40), "gauss", ACT_SIGMOID, 1.0, EPI_MUL, 128)
    add("1x3_zr", OVER, "gauss", ACT_SIGMOID, 1.0, EPI_MUL, 128)
    add("1x3_zr", RAGGED, "gauss", ACT_SIGMOID, 1.0, EPI_MUL, 128)
    add("1x3_zr", OVER, "gauss", ACT_NONE, 1.0, EPI_ADD, 128)
    add("3x3_96+64+32_384", (1, 4, 32), "exact")
    add("3x3_96+64+32_384", RAGGED, "exact", ACT_RELU)
    add("3x3_96+64+32_384", OVER, "gauss", ACT_GELU)
    add("3x3_128+128+64+64", (1, 2, 32), "exact")
    add("3x3_128+128+64+64", RAGGED, "exact", ACT_RELU)
    add("3x3_128+128+64+64", OVER, "gauss", ACT_NONE, 0.5)
    add("3x3_192", (1, 4, 40), "exact")
    add("3x3_192", RAGGED, "exact", ACT_RELU)
    add("3x3_192", OVER, "gauss", ACT_GELU)
    add("3x3_192", RAGGED, "gauss", ACT_RELU, 1.0, EPI_ADD)
    add("1x3_192+192", (1, 2, 32), "exact")
    add("1x3_192+192", RAGGED, "exact")
    add("1x3_192+192", OVER, "gauss", ACT_TANH, 1.0, EPI_GRU)
    add("1x3_192+192", RAGGED, "gauss", ACT_SIGMOID, 1.0, EPI_MUL)
    add("3x3_96+96_576", (1, 4, 32), "exact", ACT_RELU)
    add("3x3_96+96_576", RAGGED, "exact")
    add("3x3_96+96_576", OVER, "gauss", ACT_NONE)
    for layer, act in (("3x3_8+128_136", ACT_GELU), ("3x3_24_64", ACT_TANH), ("3x3_128_8", ACT_SIGMOID)):   # halo tiles only
        add(layer, (1, 4, 32), "exact")
        add(layer, RAGGED, "exact", ACT_RELU)
        add(layer, OVER, "gauss", act)
    return s


SPECS = _specs()
NAMES = tuple(SPECS)


@functools.lru_cache(maxsize=None)
def build(name, dtype="float16"):
    """built once per process and shared; nothing may write into it"""
    spec = SPECS[name]
    assert LAYERS[spec.layer].stride == 1
    return K.build_case(name, spec, LAYERS[spec.layer], dtype)


@functools.lru_cache(maxsize=None)
def reference(name, dtype="float16"):
    """computed once per process and shared"""
    return K.reference_case(build(name, dtype))


Launch = collections.namedtuple("Launch", "what korder tile PH PW CH BN")   # PH = 0: the selector chooses the patch


def launches(case):
    """every launch of a case in its dtype: the halo tiles (K order 0), then, in fp16, the fragment-stream forms (K order 2)"""
    L, out = case.layer, []
    for t in case.spec.halo:
        bn = HALO_BN.get(t, 64)                                           # (the heuristic: BN as the GPU test finds out; 64 for the gather's purposes)
        out.append(Launch(f"halo t{t}" if t else "halo auto", 0, t, 4, 32, HALO_CH[case.dtype], bn))
    if case.dtype == "float16":
        ck = frag_chunk(L)
        for t in case.spec.frag:
            ph, pw = FRAG_PATCH.get(t, (0, 0))
            out.append(Launch(f"frag {ph}x{pw}" if t else "frag auto", 2, t, ph, pw, ck, ck))
    return out


def descriptor(case, l):
    """a launch as the host program of tests/test_select_cpu.py reads it"""
    L = case.layer
    return (f"conv N={case.N} H={case.H} W={case.W} Cin={case.Cin} Cout={L.Cout} KH={L.KH} KW={L.KW} stride=1 epi={case.spec.epi} korder={l.korder} "
            f"pool2=0 ln=0 shuffle2=0 tile={l.tile} fp16={int(case.dtype == 'float16')}")


@functools.lru_cache(maxsize=None)
def selection():
    """descriptor -> what csrc/conv_select.h chooses for it ("frag 128 128 4 40 0": cout block, chunk, PH, PW, operands; "halo 64 8 4 4": BN, waves,
    WGM, weight tiles in flight), for every launch of every case in both dtypes: one run of tests/test_select_cpu.py's host program"""
    import subprocess
    import tempfile

    import test_select_cpu as S
    wanted = list(dict.fromkeys(descriptor(build(n, dt), l) for n in NAMES for dt in ("float32", "float16") for l in launches(build(n, dt))))
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = f"{tmp}/select.cpp", f"{tmp}/select"
        with open(src, "w") as f:
            f.write(S.PROGRAM)
        subprocess.run([S._compiler(), "-std=c++17", "-O1", "-I", S.ROOT, src, "-o", exe], check=True, capture_output=True, text=True)
        out = subprocess.run([exe], input="\n".join(wanted) + "\n", check=True, capture_output=True, text=True).stdout
    got = dict(ln.split(" -> ", 1) for ln in out.strip().splitlines())
    assert set(got) == set(wanted)
    return got


def chosen(case, l):
    return selection()[descriptor(case, l)]


def forced(case, l):
    """what a launch with a forced tile must select (None: the choice is the selector's), so that a line of the table names the kernel that ran"""
    if l.tile == 0:
        return None
    if l.korder == 2:
        naux = 0 if case.spec.epi == EPI_NONE else 2 if case.spec.epi in (EPI_GRU, EPI_GATEMIX) else 1
        return f"frag {l.BN} {l.CH} {l.PH} {l.PW} {naux}"
    return {12: "halo 128 4 2 1", 13: "halo 64 4 2 1", 19: "halo 128 8 2 1", 23: "halo 64 8 4 1", 24: "halo 64 8 4 4", 25: "halo 64 4 2 4",
            26: "halo 128 8 2 2"}[l.tile]


def label(case, l):
    """the launch as the table prints it: the request and the kernel conv_select.h chose for it"""
    return f"{l.what:12s} -> {chosen(case, l)}"


def forms(case):
    """the distinct (PH, PW, CH, BN) a case's launches compute on: what wrong() is evaluated for"""
    return tuple(dict.fromkeys((l.PH, l.PW, l.CH, l.BN) for l in launches(case) if l.PH))


# ---- wrong patch loaders ------------------------------------------------------------------------------------------------------------------
VARIANTS = ("image_wrap", "row_wrap", "pad_less", "stride_of_src0", "seam_zero", "chunk_tail_reads_on", "src_boundary_at_chunk", "raster_32",
            "chunk_tap_swapped", "cout_block_stride", "epi_cout0_ignored", "partial_patch_stored")
# which of (PH, PW, CH, BN) a variant's result depends on (the others: a form changes nothing, one evaluation serves them all)
DEPENDS = {"seam_zero": (0, 1), "raster_32": (0, 1), "partial_patch_stored": (0, 1), "chunk_tail_reads_on": (2,), "src_boundary_at_chunk": (2,),
           "chunk_tap_swapped": (2,), "cout_block_stride": (3,)}


def _stray_stores(case, PH, PW):
    """(image, row, column) of the patch pixels outside the image whose raster address (n H + y) W + x lies inside the output"""
    N, H, W = case.N, case.H, case.W
    Hg, Wg = -(-H // PH) * PH, -(-W // PW) * PW
    return [(n, y, x) for n in range(N) for y in range(Hg) for x in range(Wg) if (y >= H or x >= W) and (n * H + y) * W + x < N * H * W]


def differs(case, variant, PH, PW, CH, BN=None):
    """the variant computes something else than the layer on this case with patches of PH x PW, chunks of CH and cout blocks of BN, by construction"""
    L, BN = case.layer, BN or CH
    bounds = [sum(L.cs[:i]) for i in range(1, len(L.cs))]
    if variant == "image_wrap":                                          # (into the NaN images of wide(), or into the neighbouring image)
        return L.KH >= 3
    if variant == "row_wrap":
        return L.KW >= 3
    if variant == "pad_less":
        return True
    if variant == "stride_of_src0":
        return any(c != L.cs[0] for c in L.cs[1:])
    if variant == "seam_zero":                                           # more than one patch on an axis the kernel has taps on
        return (L.KW >= 3 and case.W > PW) or (L.KH >= 3 and case.H > PH)
    if variant == "chunk_tail_reads_on":
        return case.Cin % CH != 0
    if variant == "src_boundary_at_chunk":
        return any(b % CH for b in bounds)
    if variant == "raster_32":                                           # a pixel of raster index 32 or more inside the image
        return PW == 40 and (case.H > 1 or case.W > 32)
    if variant == "chunk_tap_swapped":
        return case.Cin > CH
    if variant == "cout_block_stride":
        return L.Cout > BN
    if variant == "epi_cout0_ignored":
        return case.spec.epi_cout0 > 0
    if variant == "partial_patch_stored":
        return bool(_stray_stores(case, PH, PW))
    raise KeyError(variant)


def _flat(t):
    """an operand as the device holds it: wide()'s buffer flattened, the offset of the view's first element, the pixel stride"""
    big = K.widen(t).double()
    st = big.shape[-1]
    return big.reshape(-1), big.shape[1] * big.shape[2] * st + K.PAD, st


def wrong(case, variant=None, PH=4, PW=32, CH=128, BN=None):
    """the layer by the explicit gather of the docstring.  variant None is the layer itself (tests/test_k5_patch_cases_cpu.py compares it with the
    reference for every form); the others are VARIANTS."""
    L, spec = case.layer, case.spec
    N, H, W, KH, KW, Cin, Cout = case.N, case.H, case.W, L.KH, L.KW, case.Cin, L.Cout
    BN = BN or CH
    assert L.stride == 1 and variant in (None,) + VARIANTS
    ntap, VEC = KH * KW, 16 // (2 if case.dtype == "float16" else 4)
    nchunk = -(-Cin // CH)
    Cp = nchunk * CH
    ph, pw = KH // 2, KW // 2
    if variant == "pad_less":
        ph, pw = max(ph - 1, 0), max(pw - 1, 0)
    stray = variant == "partial_patch_stored"
    Hg, Wg = (-(-H // PH) * PH, -(-W // PW) * PW) if stray else (H, W)  # the patch pixels that are computed (and, here, stored)
    y, x = torch.arange(Hg)[:, None], torch.arange(Wg)[None, :]
    y0, x0 = y // PH * PH, x // PW * PW                                  # patch origin
    q = (y - y0) * PW + (x - x0)                                         # pixel q of the patch = row of the MFMA tiles
    ry, rx = (q // 32, q % 32) if (variant == "raster_32" and PW == 40) else (q // PW, q % PW)
    HH, HW = KH + PH - 1, KW + PW - 1                                    # the halo tile
    # per channel of the padded K: the source it is read from, its channel there, whether anything is read at all
    starts = [sum(L.cs[:i]) for i in range(len(L.cs))]
    src_of, ch_of, read = [], [], []
    for k0 in range(0, Cp, VEC):
        sel = k0 // CH * CH if variant == "src_boundary_at_chunk" else k0
        i = max(j for j, s0 in enumerate(starts) if s0 <= sel)
        for e in range(VEC):
            src_of.append(i)
            ch_of.append(k0 + e - starts[i])
            read.append(k0 < Cin or variant == "chunk_tail_reads_on")
    src_of, ch_of, read = torch.tensor(src_of), torch.tensor(ch_of), torch.tensor(read)
    flats = [_flat(t) for t in case.xs]
    n = torch.arange(N)[:, None, None]
    X = torch.zeros(N, Hg, Wg, ntap, Cp, dtype=torch.float64)
    for ky in range(KH):
        for kx in range(KW):
            hy, hx = ry + ky, rx + kx                                    # halo pixel
            yy, xx = y0 - ph + hy, x0 - pw + hx                          # input pixel
            iny, inx, tile = (yy >= 0) & (yy < H), (xx >= 0) & (xx < W), (hy < HH) & (hx < HW)
            ok = iny & inx
            if variant == "row_wrap":
                ok = iny
            elif variant == "image_wrap":
                ok = inx
            elif variant == "seam_zero":
                ok = ok & (yy >= y0) & (yy < y0 + PH) & (xx >= x0) & (xx < x0 + PW)
            ok = (ok & tile)[None].expand(N, Hg, Wg)
            pix = (n * H + yy[None]) * W + xx[None]                      # flat index, whether inside or not
            for i, (flat, base, st) in enumerate(flats):
                ks = ((src_of == i) & read).nonzero().flatten()
                if ks.numel() == 0:
                    continue
                stride = flats[0][2] if variant == "stride_of_src0" else st
                addr = (base + pix[..., None] * stride + ch_of[ks]).clamp(0, flat.numel() - 1)
                X[:, :, :, ky * KW + kx, ks] = torch.where(ok[..., None], flat[addr], torch.zeros((), dtype=torch.float64))
    wm = torch.zeros(Cout, ntap, Cp, dtype=torch.float64)
    wm[:, :, :Cin] = case.w.double().permute(0, 2, 3, 1).reshape(Cout, ntap, Cin)
    b = case.b.double()
    if variant == "chunk_tap_swapped":                                   # K step (chunk c, tap t) takes the stream's step t * nchunk + c
        w4 = wm.reshape(Cout, ntap, nchunk, CH)
        sw = torch.empty_like(w4)
        for c in range(nchunk):
            for t in range(ntap):
                c2, t2 = divmod(t * nchunk + c, ntap)
                sw[:, t, c] = w4[:, t2, c2]
        wm = sw.reshape(Cout, ntap, Cp)
    if variant == "cout_block_stride":
        co = torch.arange(Cout) % BN
        wm, b = wm[co], b[co]
    pre = (X.reshape(-1, ntap * Cp) @ wm.reshape(Cout, -1).T).reshape(N, Hg, Wg, Cout) + b
    out = pre[:, :H, :W]
    if stray:                                                            # the stores of pixels outside the image land last
        out = out.clone().reshape(N * H * W, Cout)
        for (ni, yi, xi) in _stray_stores(case, PH, PW):
            out[(ni * H + yi) * W + xi] = pre[ni, yi, xi]
        out = out.reshape(N, H, W, Cout)
    if variant == "epi_cout0_ignored" and spec.epi_cout0:               # aux0's base lies epi_cout0 elements before its first element: every cout indexes it
        flat, base, st = _flat(case.a0)
        m = torch.arange(N * H * W)[:, None]
        a = flat[(base - spec.epi_cout0 + m * st + torch.arange(Cout)[None, :]).clamp(0, flat.numel() - 1)].reshape(N, H, W, Cout)
        v = K.activate(out, spec.act) * spec.scale
        return (v + a if spec.epi == EPI_ADD else v * a) + 0.0
    return K.finish(case, out) + 0.0
