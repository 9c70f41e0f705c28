"""ctypes binding of libssdk.so (C-ABI: include/ssdk.h) -- the only door to the HIP kernels.

There is NO fallback: if the shared library is missing or a call fails, an exception is raised.
Tensors are passed as raw ``data_ptr()`` values plus the caller's current HIP stream, so every call is
asynchronous and hipGraph-capturable.  This module is the `ssds._C` the reference names but never
ships (reference ssds/modeling/layers/box.py:3-4, 419-421, 483-485).
"""
import collections
import ctypes
import os
import re
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "csrc", "libssdk.so")
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "ssdk.h")

# ---- include/ssdk.h is the one description of the C ABI: prototypes, descriptor structs and constants are read from it ----

Header = collections.namedtuple("Header", "constants structs functions")

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_FIELDS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
_POINTER = re.compile(r"([A-Za-z_][\w ]*?)\s*(\*[\s*]*)([A-Za-z_]\w*)?$")  # pointee words, stars, optional name
_SCALAR = re.compile(r"(\w+)(?:\s+[A-Za-z_]\w*)?$")  # type word, optional name: `float x[4]` (a pointer in C) does not match


def _refuse(what, decl):
    raise ImportError("include/ssdk.h: {} in `{}` -- ssds/_native.py binds the types of its whitelist only".format(
        what, " ".join(decl.split())))


def _param_type(text, structs, decl):
    """ctypes type of one parameter (`const float* w`, `size_t n`, `const ssdk_level* levels`)."""
    text = re.sub(r"\bconst\b", " ", text).strip()
    m = _POINTER.match(text)
    if m:
        pointee = " ".join(m.group(1).split())
        if pointee in structs and m.group(2).count("*") == 1:
            return ctypes.POINTER(structs[pointee])
        return ctypes.c_void_p
    m = _SCALAR.match(text)
    if not m or m.group(1) not in _SCALARS:
        _refuse("parameter `{}` has no ctypes counterpart".format(text), decl)
    return _SCALARS[m.group(1)]


def _return_type(text, opaque, decl):
    text = " ".join(re.sub(r"\bconst\b", " ", text).replace("*", " * ").split())
    if text in ("int", "size_t"):
        return _SCALARS[text]
    if text == "void":
        return None
    if text == "char *":
        return ctypes.c_char_p
    if text.endswith(" *") and text[:-2] in opaque:
        return ctypes.c_void_p
    _refuse("return type `{}` has no ctypes counterpart".format(text), decl)


def _struct_fields(body, constants, structs, decl):
    fields = []
    for member in filter(None, (m.strip() for m in body.split(";"))):
        text = re.sub(r"\bconst\b", " ", member).strip()
        m = _POINTER.match(text)
        if m:
            if not m.group(3):
                _refuse("member `{}` has no name".format(member), decl)
            fields.append((m.group(3), ctypes.c_void_p))
            continue
        ctype, _, names = text.partition(" ")
        base = _FIELDS.get(ctype) or structs.get(ctype)
        if base is None or not names.strip():
            _refuse("member `{}` has no ctypes counterpart".format(member), decl)
        for name in names.split(","):
            m = re.match(r"\s*(\w+)\s*(?:\[\s*(?:(SSDK_\w+)\s*\*\s*)?(\d+)\s*\])?\s*$", name)
            if not m or (m.group(2) and m.group(2) not in constants):
                _refuse("member `{}` has a declarator outside `name` / `name[N]` / `name[SSDK_X * N]`".format(member), decl)
            if m.group(3) is None:
                fields.append((m.group(1), base))
            else:
                fields.append((m.group(1), base * (constants.get(m.group(2), 1) * int(m.group(3)))))
    return fields


def parse_header(text, struct_names=None):
    """The C ABI that header text declares: ``constants`` {SSDK_X: int} from the #defines and the enums (decimal integers),
    ``structs`` {typedef name: ctypes.Structure} (class names from ``struct_names``, else the typedef's) and ``functions``
    {name: (restype, argtypes)}, each in header order.  Anything the closed type whitelist cannot express is an ImportError
    quoting the declaration -- never skipped, never defaulted: a wrong width here is a truncated device address."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants, structs, functions, opaque = {}, collections.OrderedDict(), collections.OrderedDict(), set()
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SSDK_\w+)(.*)$", text, flags=re.M):
        if value.strip():  # the include guard has none
            if not re.match(r"\s+-?\d+\s*$", value):
                _refuse("the value is not a decimal integer", "#define " + name + value)
            constants[name] = int(value)
    text = re.sub(r"#\s*ifdef\s+__cplusplus.*?#\s*endif", " ", text, flags=re.S)  # extern "C" { ... }
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    def enum(m):
        for entry in filter(None, (e.strip() for e in m.group(1).split(","))):
            e = re.match(r"(SSDK_\w+)\s*=\s*(-?\d+)$", entry)
            if not e:
                _refuse("enumerator `{}` has no literal value".format(entry), m.group(0))
            constants[e.group(1)] = int(e.group(2))
        return " "

    text = re.sub(r"(?:typedef\s+)?enum\s*\{([^}]*)\}\s*\w*\s*;", enum, text)

    def opaque_struct(m):
        opaque.add(m.group(1))
        return " "

    text = re.sub(r"typedef\s+struct\s+\w+\s+(\w+)\s*;", opaque_struct, text)
    # structs and prototypes in one pass, in header order: a prototype may only point to a struct defined above it
    pos = 0
    for m in re.finditer(r"typedef\s+struct\s+\w*\s*\{([^}]*)\}\s*(\w+)\s*;|([^;{}]*[^;{}\s][^;{}]*);", text):
        if text[pos:m.start()].strip():
            _refuse("text that is neither a declaration nor a typedef", text[pos:m.start()])
        pos = m.end()
        decl = m.group(0)
        if m.group(2):
            cname = m.group(2)
            structs[cname] = type((struct_names or {}).get(cname, cname), (ctypes.Structure,),
                                  {"_fields_": _struct_fields(m.group(1), constants, structs, decl)})
            continue
        f = re.match(r"\s*(.*?)\b(ssdk_\w+)\s*\((.*)\)\s*$", m.group(3), flags=re.S)
        if not f or not f.group(1).strip():
            _refuse("not a function prototype", decl)
        params = f.group(3).strip()
        functions[f.group(2)] = (_return_type(f.group(1), opaque, decl),
                                 [] if params == "void" else [_param_type(p, structs, decl) for p in params.split(",")])
    if text[pos:].strip():
        _refuse("text that is neither a declaration nor a typedef", text[pos:])
    return Header(constants, structs, functions)


# Every header under include/, ssdk.h first: (file name, {typedef name in the header: the mirror's name here}).  The kernels added
# after ABI 245 have headers of their own -- the entry points of ssdk.h and the layout of ssdk_op are a closed list under it -- read
# with the same parser; a new header is one entry here (plus the names it exports below).
_MIRRORS = collections.OrderedDict((
    ("ssdk_level", "Level"), ("ssdk_conv_desc", "ConvDesc"), ("ssdk_mbconv_desc", "MbConvDesc"), ("ssdk_fuse_desc", "FuseDesc"),
    ("ssdk_stem_desc", "StemDesc"), ("ssdk_pool_desc", "PoolDesc"), ("ssdk_xpair_desc", "XpairDesc"),
    ("ssdk_augment_desc", "AugmentDesc"), ("ssdk_mbse_desc", "MbSeDesc"), ("ssdk_op", "Op")))
_HEADERS = (
    ("ssdk.h", _MIRRORS),
    ("ssdk_convt.h", {"ssdk_convt_desc": "ConvTDesc"}),  # the transposed convolution of the Shelf neck
    ("ssdk_cat.h", {"ssdk_cat_desc": "CatDesc", "ssdk_spp_desc": "SppDesc"}),  # channel concatenation and SPP block of the YOLO necks
    ("ssdk_dkres.h", {"ssdk_dkres_desc": "DkresDesc"}),  # the DarkNet residual block as one launch
    ("ssdk_dconv.h", {}),  # the dilated 3x3 convolution of the RFB extras (described by ssdk_conv_desc: no descriptor of its own)
    # the DenseNet dense layer as one launch, the front of a transition and the copy into a block's buffer
    ("ssdk_denselayer.h", {"ssdk_dense_layer_desc": "DenseLayerDesc", "ssdk_dense_pool_desc": "DensePoolDesc",
                           "ssdk_dense_place_desc": "DensePlaceDesc"}),
    # the ShuffleNetV2 unit as one launch, stride 1 and stride 2
    ("ssdk_shuffle.h", {"ssdk_shuffle_unit_desc": "ShuffleUnitDesc", "ssdk_shuffle_down_desc": "ShuffleDownDesc"}),
    ("ssdk_cattrain.h", {}),  # cat / SPP of the YOLO TRAINING step, forward and backward on NCHW tensors (no descriptors)
    ("ssdk_convttrain.h", {}),  # the transposed 3x3 / stride 2 of the Shelf TRAINING step, forward and gradients on NCHW tensors
    ("ssdk_shuffletrain.h", {}),  # the ShuffleNetV2 TRAINING step: 1x1 on channel slices of any width, the interleaving join
    ("ssdk_densetrain.h", {}),  # the DenseNet dense-block TRAINING step on one buffer: place + sums, 1x1 with norm1 on load, norm1 backward
    ("ssdk_apsweep.h", {}),  # average precision over a sweep of IoU thresholds (AP@[.50:.95]): the reference's rule or the COCO rule
    ("ssdk_cocoeval.h", {}),  # the COCO detection summary: area ranges, crowd boxes, maxDets per image and category, recall
    ("ssdk_variant.h", {}),  # ssdk_last_variant: the template instance behind ssdk_last_kernel's name (tests, tools)
)
# the library first: without it nothing below matters, and its message says how to build it -- no header error may mask it
if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libssdk.so not found at {} -- build it first: `python -c 'import __graft_entry__ as g; "
        "g.build()'` or `make -C ssds.pytorch_amd/csrc` (there is no CPU fallback)".format(LIB_PATH)
    )
_PATHS = [os.path.join(os.path.dirname(HEADER_PATH), _name) for _name, _ in _HEADERS]
_PARSED = []
_ABI = Header({}, collections.OrderedDict(), collections.OrderedDict())  # every header's declarations in one place
for _path, (_name, _mirrors) in zip(_PATHS, _HEADERS):
    if not os.path.exists(_path):
        raise ImportError("include/{} not found at {} -- ssds/_native.py reads the C ABI of libssdk.so from it".format(_name, _path))
    with open(_path) as _f:
        _PARSED.append(parse_header(_f.read(), _mirrors))
    for _merged, _part in zip(_ABI, _PARSED[-1]):
        _merged.update(_part)
_K = _ABI.constants

ABI_VERSION = _K["SSDK_VERSION"]  # a library of an older version is refused by _load
(EXPORTS, CONVT_EXPORTS, CAT_EXPORTS, DKRES_EXPORTS, DCONV_EXPORTS, DENSE_EXPORTS, SHUFFLE_EXPORTS, CATTRAIN_EXPORTS,
 CONVTTRAIN_EXPORTS, SHUFFLETRAIN_EXPORTS, DENSETRAIN_EXPORTS, APSWEEP_EXPORTS, COCOEVAL_EXPORTS, VARIANT_EXPORTS) = (tuple(_h.functions) for _h in _PARSED)
(_, CONVT_HEADER_PATH, CAT_HEADER_PATH, DKRES_HEADER_PATH, DCONV_HEADER_PATH, DENSE_HEADER_PATH, SHUFFLE_HEADER_PATH, CATTRAIN_HEADER_PATH,
 CONVTTRAIN_HEADER_PATH, SHUFFLETRAIN_HEADER_PATH, DENSETRAIN_HEADER_PATH, APSWEEP_HEADER_PATH, COCOEVAL_HEADER_PATH, VARIANT_HEADER_PATH) = _PATHS

MAX_LEVELS, MAX_ANCHORS, MAX_TOPN, MAX_NDET, MAX_NMS_N, MAX_GT = (
    _K["SSDK_MAX_" + n] for n in ("LEVELS", "ANCHORS", "TOPN", "NDET", "NMS_N", "GT"))
F32, BF16, F16 = _K["SSDK_F32"], _K["SSDK_BF16"], _K["SSDK_F16"]
ACT = {n: _K["SSDK_ACT_" + n.upper()] for n in ("none", "relu", "relu6", "silu", "sigmoid")}
_DTYPES = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
U8 = _K["SSDK_U8"]  # ssdk_preprocess source only
OP_CONV, OP_MBCONV, OP_FUSE, OP_STEM7, OP_POOL, OP_XPAIR, OP_MBSE, OP_CONVT, OP_CAT, OP_SPP, OP_DKRES = (
    _K["SSDK_OP_" + n] for n in ("CONV", "MBCONV", "FUSE", "STEM7", "POOL", "XPAIR", "MBSE", "CONVT", "CAT", "SPP", "DKRES"))
OP_DENSE, OP_DENSEPOOL, OP_DENSEPLACE = (_K["SSDK_OP_" + n] for n in ("DENSE", "DENSEPOOL", "DENSEPLACE"))
OP_SHUFFLE, OP_SHUFFLEDOWN = _K["SSDK_OP_SHUFFLE"], _K["SSDK_OP_SHUFFLEDOWN"]
MBSE_DW, MBSE_GATE, MBSE_PROJ = 1, 2, 4  # ssdk_mbse_desc.stages bits (0 = all three); the header has no names for them
FUSE_SAME, FUSE_UP2, FUSE_POOL2 = _K["SSDK_FUSE_SAME"], _K["SSDK_FUSE_UP2"], _K["SSDK_FUSE_POOL2"]
NCHW, NHWC = _K["SSDK_LAYOUT_NCHW"], _K["SSDK_LAYOUT_NHWC"]

Level, ConvDesc, MbConvDesc, FuseDesc, StemDesc, PoolDesc, XpairDesc, AugmentDesc, MbSeDesc, Op = (
    _ABI.structs[cname] for cname in _MIRRORS)
ConvTDesc, CatDesc, SppDesc, DkresDesc = (_ABI.structs["ssdk_%s_desc" % n] for n in ("convt", "cat", "spp", "dkres"))
DenseLayerDesc, DensePoolDesc, DensePlaceDesc = (_ABI.structs["ssdk_dense_%s_desc" % n] for n in ("layer", "pool", "place"))
ShuffleUnitDesc, ShuffleDownDesc = _ABI.structs["ssdk_shuffle_unit_desc"], _ABI.structs["ssdk_shuffle_down_desc"]
AugmentDesc.__doc__ = ("ssdk_augment_desc: one image of an ssdk_augment batch (ssds/dataset/augment.py DESC_DTYPE is the numpy "
                       "view of it).")
MbSeDesc.__doc__ = "ssdk_mbse_desc: the tail of an EfficientNet MBConv block (depthwise + SE gate + gated projection)."
ConvTDesc.__doc__ = "ssdk_convt_desc: transposed 3x3 / stride 2 / pad 1 convolution + bias (+ skip), the Shelf decoder step."
CatDesc.__doc__ = "ssdk_cat_desc: y = a || b, or a || nearest_x2(b), along the channels (YOLOv3 / PAN concatenations)."
SppDesc.__doc__ = "ssdk_spp_desc: y = x || maxpool5(x) || maxpool9(x) || maxpool13(x) (the SPP block of YOLOv4)."
DkresDesc.__doc__ = "ssdk_dkres_desc: y = x + act2(bn2(conv3x3(act1(bn1(conv1x1(x)))))), the DarkNet residual block in one launch."
DenseLayerDesc.__doc__ = ("ssdk_dense_layer_desc: y[Cin : Cin + 32] = conv3x3(relu(bn2(conv1x1(relu(bn1(x[:Cin])))))) in one launch, x and y "
                          "in one buffer of pixel stride ld.")
DensePoolDesc.__doc__ = "ssdk_dense_pool_desc: y = avgpool2x2(relu(a * x + b)), x with pixel stride ld (the front of a DenseNet transition)."
DensePlaceDesc.__doc__ = "ssdk_dense_place_desc: a dense NHWC tensor copied into channels [0, C) of a buffer with pixel stride ld."
ShuffleUnitDesc.__doc__ = ("ssdk_shuffle_unit_desc: y[2i] = x[i], y[2i + 1] = branch2(x[Cb:])[i] -- the stride-1 ShuffleNetV2 unit in one "
                           "launch, the channel shuffle in the store.")
ShuffleDownDesc.__doc__ = "ssdk_shuffle_down_desc: y[2i] = branch1(x)[i], y[2i + 1] = branch2(x)[i] -- the stride-2 unit in one launch."
DKRES_TILE_H, DKRES_TILE_W = _K["SSDK_DKRES_TILE_H"], _K["SSDK_DKRES_TILE_W"]  # a workgroup's output tile
# the dilation field of ssdk_conv_desc.res_mode and the dilated kernel's tiling (include/ssdk_dconv.h)
CONV_DILATION_SHIFT, CONV_DILATION_MASK = _K["SSDK_CONV_DILATION_SHIFT"], _K["SSDK_CONV_DILATION_MASK"]
DCONV_TILE_PIXELS, DCONV_FRAG_COUT, DCONV_TILE_COUT, DCONV_KSPLIT = (
    _K["SSDK_DCONV_" + n] for n in ("TILE_PIXELS", "FRAG_COUT", "TILE_COUT", "KSPLIT"))
DCONV_MIN_DILATION, DCONV_MAX_DILATION, DCONV_MAX_CHANNELS, DCONV_MAX_SIDE = (
    _K["SSDK_DCONV_" + n] for n in ("MIN_DILATION", "MAX_DILATION", "MAX_CHANNELS", "MAX_SIDE"))
DENSE_TILE_H, DENSE_TILE_W = _K["SSDK_DENSE_TILE_H"], _K["SSDK_DENSE_TILE_W"]
DENSE_CMID, DENSE_COUT = _K["SSDK_DENSE_CMID"], _K["SSDK_DENSE_COUT"]
SHUFFLE_TILE_H, SHUFFLE_TILE_W = _K["SSDK_SHUFFLE_TILE_H"], _K["SSDK_SHUFFLE_TILE_W"]
SHUFFLE_DOWN_TILE_H, SHUFFLE_DOWN_TILE_W = _K["SSDK_SHUFFLE_DOWN_TILE_H"], _K["SSDK_SHUFFLE_DOWN_TILE_W"]
SHUFFLE_CHUNK = _K["SSDK_SHUFFLE_CHUNK"]  # weight images and vectors are zero-padded to a multiple of it
SPP_TRAIN_MAX_SIDE = _K["SSDK_SPP_TRAIN_MAX_SIDE"]  # the largest H / W ssdk_spp_train_* stage in LDS
APSWEEP_MAX_T = _K["SSDK_APSWEEP_MAX_T"]  # IoU thresholds per ssdk_apsweep_match launch (include/ssdk_apsweep.h)
AP_RULE = {"reference": _K["SSDK_AP_RULE_REFERENCE"], "coco": _K["SSDK_AP_RULE_COCO"]}
# IoU thresholds, area ranges and maxDets values per ssdk_cocoeval_* call (include/ssdk_cocoeval.h)
COCOEVAL_MAX_T, COCOEVAL_MAX_A, COCOEVAL_MAX_M = (_K["SSDK_COCOEVAL_MAX_" + n] for n in "TAM")


def _load():
    lib = ctypes.CDLL(LIB_PATH)

    def bind(name):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ABI.functions[name]
        return fn

    # version FIRST: a library older than ABI 230 has no ssdk_struct_size, and a bare AttributeError from the symbol lookup
    # below would hide what is wrong
    try:
        have = int(bind("ssdk_version")())
    except AttributeError:
        have = 0
    if have < ABI_VERSION:
        raise ImportError("libssdk.so at {} is ABI {} but ssds/_native.py is written for ABI {}: rebuild it "
                          "(`make -C ssds.pytorch_amd/csrc`)".format(LIB_PATH, have, ABI_VERSION))
    for name in _ABI.functions:
        try:
            bind(name)
        except AttributeError:
            raise ImportError("libssdk.so at {} does not export {}, which include/ssdk.h (or {} next to it) declares: rebuild it "
                              "(`make -C ssds.pytorch_amd/csrc`)".format(LIB_PATH, name, ", ".join(n for n, _ in _HEADERS[1:])))
    # the ctypes mirrors must have the layout the library was BUILT with: a shorter struct would be read past its end.
    # SSDK_SIZEOF_X is the index of struct ssdk_x
    for key, which in sorted((kv for kv in _K.items() if kv[0].startswith("SSDK_SIZEOF_")), key=lambda kv: kv[1]):
        cls = _ABI.structs["ssdk_" + key[len("SSDK_SIZEOF_"):].lower()]
        want = lib.ssdk_struct_size(which)
        if want != ctypes.sizeof(cls):
            raise ImportError("libssdk.so at {} was built against another include/ssdk.h: sizeof({}) is {} there, {} in ssds/_native.py"
                              .format(LIB_PATH, cls.__name__, want, ctypes.sizeof(cls)))
    if lib.ssdk_abi_check(ABI_VERSION, ctypes.sizeof(Op)) != 0:
        raise ImportError("libssdk.so at {}: {}".format(LIB_PATH, lib.ssdk_last_error().decode()))
    # the structs that are not behind ssdk_struct_size (its eight indices are part of ABI 245) have an entry point that reports
    # their size: ssdk_x_desc -> ssdk_x_desc_bytes
    for cname, cls in _ABI.structs.items():
        if cname + "_bytes" in _ABI.functions:
            want = int(getattr(lib, cname + "_bytes")())
            if want != ctypes.sizeof(cls):
                raise ImportError("libssdk.so at {} has sizeof({}) = {} but ssds/_native.py mirrors it with {} bytes: "
                                  "rebuild it (`make -C ssds.pytorch_amd/csrc`)".format(LIB_PATH, cname, want, ctypes.sizeof(cls)))
    return lib


lib = _load()


class Context(object):
    """A caller-owned ``ssdk_ctx`` (include/ssdk.h "Contexts"): the HIP objects behind the multi-launch entry points
    (side stream + fork/join events of the plan executor, tail-stream fork events and the profiling rings of the
    decode stage).  Bound to the device that is current when it is created; used by one host thread at a time --
    every ``Decoder`` and every ``ConvPlan`` owns one, so two threads / two devices share no state."""

    def __init__(self, device):
        self.device = torch.device(device)
        with torch.cuda.device(self.device):
            self.ptr = lib.ssdk_ctx_create()
        if not self.ptr:
            raise SsdkError("ssdk_ctx_create failed: " + lib.ssdk_last_error().decode())
        self.ptr = ctypes.c_void_p(self.ptr)

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                lib.ssdk_ctx_destroy(self.ptr)
                self.ptr = None
        except Exception:  # interpreter shutdown
            pass

    def _call(self, fn, *a):
        with torch.cuda.device(self.device):
            return fn(self.ptr, *a)

    def set_tail_stream(self, stream):
        check(self._call(lib.ssdk_ctx_set_tail_stream, ctypes.c_void_p(stream.cuda_stream) if stream is not None else None),
              "ctx_set_tail_stream")

    def set_side_lane(self, on):
        """True / False: the caller's explicit choice (a plan with side-stream chains respects it); None: back to the default
        (SSDK_SIDE_STREAM, and a plan that recorded side-stream chains turns the lane on again by itself)."""
        self.side_user = None if on is None else bool(on)
        self.side_auto = False
        check(self._call(lib.ssdk_ctx_set_side_lane, -1 if on is None else int(bool(on))), "ctx_set_side_lane")

    def auto_side_lane(self):
        """A plan whose small pyramid levels were recorded for the side stream (fused_conv.ConvPlan.launch): on, unless the
        caller chose (set_side_lane True / False) or the environment says SSDK_SIDE_STREAM=0."""
        if getattr(self, "side_user", None) is not None or getattr(self, "side_auto", False):
            return
        if os.environ.get("SSDK_SIDE_STREAM", "") == "0":
            return
        check(self._call(lib.ssdk_ctx_set_side_lane, 1), "ctx_set_side_lane")
        self.side_auto = True

    def set_profiling(self, on):
        """True / 1: hipEvents around every launch of the decode stage; 2: ONE interval around the whole stage (no event
        between its launches: an event costs ~4.6 us of GPU time on this stack and flushes caches between the kernels it
        separates), read back as timings_ms()[0]; False: off."""
        check(self._call(lib.ssdk_ctx_set_profiling, 2 if on == 2 else (1 if on else 0)), "ctx_set_profiling")

    def timings_ms(self, back=0):
        """(scan_kernel, tail_kernel | level_kernel, nms_kernel | 0) ms of the profiled decode_nms call ``back`` calls ago."""
        ms = (ctypes.c_float * 3)()
        check(self._call(lib.ssdk_ctx_get_timings, int(back), ms, 3), "ctx_get_timings")
        return float(ms[0]), float(ms[1]), float(ms[2])

    def set_op_profiling(self, on):
        check(self._call(lib.ssdk_ctx_set_op_profiling, 1 if on else 0), "ctx_set_op_profiling")

    def op_timings(self):
        ms = (ctypes.c_float * 128)()
        names = (ctypes.c_char_p * 128)()
        n = self._call(lib.ssdk_ctx_get_op_timings, ms, names, 128)
        if n < 0:
            raise SsdkError(lib.ssdk_last_error().decode())
        return [(names[i].decode() if names[i] else "", float(ms[i])) for i in range(n)]

    def tail_stamps(self, n=48):
        """Debug stamps (SSDK_TAIL_STAMPS=1): [0, 24) tail_kernel, [24, 48) scan kernel phases of workgroup 0 (shader clock);
        n = 48 + 2 * W also returns wall-clock (100 MHz) start / end pairs of the first W <= 4096 scan workgroups."""
        out = (ctypes.c_ulonglong * n)()
        check(self._call(lib.ssdk_ctx_get_tail_stamps, out, n), "ctx_get_tail_stamps")
        return [int(out[i]) for i in range(n)]


def op_timings():
    """[(kernel name, ms)] of the most recent ssdk_run_ops call made while op profiling was on (stream synchronised);
    the calling thread's default context (plans own their context: ``ConvPlan.ctx.op_timings()``)."""
    ms = (ctypes.c_float * 128)()
    names = (ctypes.c_char_p * 128)()
    n = lib.ssdk_get_op_timings(ms, names, 128)
    if n < 0:
        raise SsdkError(lib.ssdk_last_error().decode())
    return [(names[i].decode() if names[i] else "", float(ms[i])) for i in range(n)]


def last_kernel():
    """Name of the kernel this thread launched last (which variant a layer was dispatched to)."""
    return lib.ssdk_last_kernel().decode()


def last_variant():
    """The template instance and launcher branch behind ``last_kernel()``'s name (include/ssdk_variant.h): "<instance> | <sizes>",
    or "" for a kernel whose launcher notes none."""
    return lib.ssdk_last_variant().decode()


class SsdkError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        raise SsdkError("{} failed ({}): {}".format(what, rc, lib.ssdk_last_error().decode()))


def dtype_code(t):
    try:
        return _DTYPES[t.dtype]
    except KeyError:
        raise TypeError("unsupported dtype {} (float32, bfloat16, float16)".format(t.dtype))


def require_device(t, what):
    if not t.is_cuda:
        raise SsdkError(
            "{}: tensor is on '{}' -- the MI355X path has no CPU fallback; move it to a HIP device".format(
                what, t.device))
    return t


def stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_ws_lock = threading.Lock()
_ws = {}


def workspace(device, nbytes):
    """Grow-only per-(device, stream) scratch buffer.  Kernels are stream-ordered, so consecutive
    calls on the same stream may share it."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    nbytes = max(int(nbytes), 256)
    with _ws_lock:
        buf = _ws.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, device=device)
            _ws[key] = buf
    return buf


_scratch = {}


def scratch(device, user, nbytes):
    """Zero-filled, grow-only per-(device, stream) scratch holding arrival counters (split-K slabs, BatchNorm tickets).  The
    kernels leave their counters at zero, so calls in stream order may share it, and calls on other streams get their own.
    ``user`` keys one counter layout: users whose layouts differ never share a buffer."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, user)
    with _ws_lock:
        buf = _scratch.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.zeros(int(nbytes), dtype=torch.uint8, device=device)
            _scratch[key] = buf
    return buf


def make_level(cls, box, stride, anchors):
    """anchors: CPU float tensor / ndarray [A,4].  cls [B, A*C, H, W], box [B, A*4, H, W]."""
    import numpy as np

    anc = np.ascontiguousarray(
        anchors.detach().cpu().numpy() if torch.is_tensor(anchors) else anchors, dtype=np.float32)
    A = int(anc.shape[0])
    if A > MAX_ANCHORS:
        raise SsdkError("at most {} anchors per location (got {})".format(MAX_ANCHORS, A))
    if cls.shape[1] % A or box.shape[1] != 4 * A:
        raise SsdkError("head channels {} / {} do not match {} anchors".format(cls.shape[1], box.shape[1], A))
    lv = Level()
    lv.cls = cls.data_ptr()
    lv.box = box.data_ptr()
    lv.A = A
    lv.C = int(cls.shape[1] // A)
    lv.H, lv.W = int(cls.shape[-2]), int(cls.shape[-1])
    lv.stride = int(stride)
    flat = anc.reshape(-1)
    for i in range(flat.shape[0]):
        lv.anchors[i] = float(flat[i])
    return lv


def set_profiling(on):
    check(lib.ssdk_set_profiling(1 if on else 0), "set_profiling")


def timings_ms(back=0):
    """(scan_kernel, tail_kernel | level_kernel, nms_kernel | 0) milliseconds of the profiled decode_nms call `back`
    calls before the most recent one (the calling thread's default context; a ``Decoder`` owns its own)."""
    ms = (ctypes.c_float * 3)()
    check(lib.ssdk_get_timings(int(back), ms, 3), "get_timings")
    return float(ms[0]), float(ms[1]), float(ms[2])


def device_info():
    cu, khz, mem = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    arch = ctypes.create_string_buffer(64)
    check(lib.ssdk_device_info(ctypes.byref(cu), ctypes.byref(khz), ctypes.byref(mem), arch, 64), "device_info")
    return {"cu_count": cu.value, "clock_khz": khz.value, "hbm_bytes": mem.value, "arch": arch.value.decode()}
