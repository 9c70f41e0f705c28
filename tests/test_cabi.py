"""CPU-side checks of the C-ABI library (no GPU compute): it loads, exports every symbol that
include/ssdk.h declares, the host-only entry points are bit-exact with the reference fixtures, and
bad arguments come back as error codes with a message (never a crash)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_exported():
    from ssds import _native as N

    hdr = open(os.path.join(ROOT, "include", "ssdk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ssdk_[a-z_0-9]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    assert declared == set(N.EXPORTS), declared ^ set(N.EXPORTS)
    for name in declared:
        assert hasattr(N.lib, name), name
    assert N.lib.ssdk_version() == 245 == N.ABI_VERSION


def test_descriptor_layouts_are_the_ones_the_library_was_built_with():
    """ssdk_struct_size (version 230): the ctypes mirrors of every descriptor struct have the size the library reports (the
    loader refuses to import otherwise), an unknown index reports 0, and the C compiler agrees with both about the header.
    Sizes do not see two swapped members of one width, so the compiler's offsetof of every member of ssdk_conv_desc and
    ssdk_op is compared with the mirrors' too."""
    import subprocess
    import tempfile

    from ssds import _native as N

    classes = (N.Level, N.ConvDesc, N.MbConvDesc, N.FuseDesc, N.StemDesc, N.PoolDesc, N.XpairDesc, N.Op)
    sizes = [int(N.lib.ssdk_struct_size(i)) for i in range(len(classes))]
    assert sizes == [ctypes.sizeof(c) for c in classes] and all(sizes)
    assert N.lib.ssdk_struct_size(len(classes)) == 0 and N.lib.ssdk_struct_size(-1) == 0
    src = ('#include <stdio.h>\n#include "ssdk.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ssdk_level), '
           "sizeof(ssdk_conv_desc), sizeof(ssdk_mbconv_desc), sizeof(ssdk_fuse_desc), sizeof(ssdk_stem_desc), sizeof(ssdk_pool_desc), "
           "sizeof(ssdk_xpair_desc), sizeof(ssdk_op));\n")
    mirrors = (("ssdk_conv_desc", N.ConvDesc), ("ssdk_op", N.Op))
    members = [(cname, f[0]) for cname, cls in mirrors for f in cls._fields_]
    src += "".join('printf(" %zu", offsetof({}, {}));\n'.format(*m) for m in members) + 'printf("\\n"); return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")], check=True)
        out, offsets = subprocess.run([os.path.join(d, "s")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert [int(v) for v in out.split()] == sizes
    assert len(members) == 23 + 9 and N.Op._fields_[2] == ("conv", N.ConvDesc)
    assert [int(v) for v in offsets.split()] == [getattr(cls, f[0]).offset for _, cls in mirrors for f in cls._fields_]


def test_abi_check_rejects_another_header():
    """ssdk_abi_check (version 240): the library accepts the header it was built with (any last digit of the version) and
    rejects a caller compiled for another minor version or with another sizeof(ssdk_op) -- with a message, not a crash."""
    from ssds import _native as N

    sz = ctypes.sizeof(N.Op)
    assert N.lib.ssdk_abi_check(N.ABI_VERSION, sz) == 0
    assert N.lib.ssdk_abi_check(N.ABI_VERSION // 10 * 10 + 9, sz) == 0
    assert N.lib.ssdk_abi_check(N.ABI_VERSION - 10, sz) == -1 and b"ABI" in N.lib.ssdk_last_error()
    assert N.lib.ssdk_abi_check(N.ABI_VERSION, sz - 8) == -1 and b"sizeof" in N.lib.ssdk_last_error()


def test_library_is_in_tree_and_has_gfx950_code():
    from ssds import _native as N

    assert N.LIB_PATH.startswith(ROOT)
    blob = open(N.LIB_PATH, "rb").read()
    assert b"gfx950" in blob


def test_generate_anchors_bit_exact_with_reference_fixture(golden_dir):
    from ssds.modeling.layers import box

    g = np.load(os.path.join(golden_dir, "anchors.npz"))
    for k in g.files:
        if k.endswith("_spec"):
            continue
        spec = g[k + "_spec"]
        s, nr, ns = int(spec[0]), int(spec[1]), int(spec[2])
        r = [float(v) for v in spec[3:3 + nr]]
        sc = [float(v) for v in spec[3 + nr:3 + nr + ns]]
        got = box.generate_anchors(s, r, sc)
        assert got.dtype.is_floating_point and tuple(got.shape) == (nr * ns, 4)
        np.testing.assert_array_equal(got.numpy(), g[k], err_msg=k)


def test_bad_arguments_return_codes():
    from ssds import _native as N

    out = (ctypes.c_float * 4)()
    assert N.lib.ssdk_generate_anchors(0, out, 1, out, 1, out) == -1
    assert b"generate_anchors" in N.lib.ssdk_last_error()
    lv = N.Level()
    lv.A, lv.C, lv.H, lv.W, lv.stride = 3, 5, 7, 9, 8
    # top_n beyond the documented limit -> workspace query refuses (0) and decode returns BADARG
    assert N.lib.ssdk_decode_workspace_bytes(ctypes.byref(lv), 1, 2, 0, 5000) == 0
    assert N.lib.ssdk_decode(ctypes.byref(lv), 2, 0, 0.05, 5000, 1, None, None, None, None, 0, None) == -1
    assert N.lib.ssdk_decode_workspace_bytes(ctypes.byref(lv), 1, 2, 0, 50) > 0
    # null pointers
    assert N.lib.ssdk_nms(None, None, None, 1, 10, 0.5, 5, 1, None, None, None, None, 0, None) == -1
    assert N.lib.ssdk_match_targets(None, 1, 1, out, 1, 1, 1, 1, 8, 0.5, 0.4, 0.0, None, None, None, None) == -1


def test_no_cpu_fallback():
    import torch
    from ssds import _native as N
    from ssds.modeling.layers import box

    cls = torch.zeros(1, 2, 2, 2)
    loc = torch.zeros(1, 4, 2, 2)
    anc = torch.tensor([[-4.0, -4, 11, 11]])
    with pytest.raises(N.SsdkError, match="no CPU fallback"):
        box.decode(cls, loc, 8, 0.05, 10, anc)
    with pytest.raises(N.SsdkError, match="no CPU fallback"):
        box.nms(torch.zeros(1, 4), torch.zeros(1, 4, 4), torch.zeros(1, 4))


def test_no_cpu_fallback_for_training_and_eval_kernels():
    """The fused loss, the mAP bookkeeping, target assignment and the fused conv entry points refuse host tensors."""
    from collections import OrderedDict

    import torch
    from ssds import _native as N
    from ssds.core.evaluation_metrics import MeanAveragePrecision
    from ssds.core.fused_loss import match_loss
    from ssds.modeling.layers import box

    anchors = OrderedDict([(8, torch.tensor([[-4.0, -4, 11, 11]]))])
    targets = torch.tensor([[[1.0, 1, 8, 8, 0]]])
    with pytest.raises(N.SsdkError, match="no CPU fallback"):
        match_loss(torch.zeros(1, 3, 2, 2), torch.zeros(1, 4, 2, 2), targets, anchors, 3, 8, [0.5, 0.4])
    with pytest.raises(N.SsdkError, match="no CPU fallback"):
        box.extract_targets(targets, anchors, 3, 8, (2, 2), [0.5, 0.4])
    with pytest.raises(N.SsdkError, match="no CPU fallback"):
        MeanAveragePrecision(3, 0.1, 0.5)((torch.zeros(1, 4), torch.zeros(1, 4, 4), torch.zeros(1, 4)), targets)
    # bad arguments come back as error codes, not crashes
    assert N.lib.ssdk_match_loss(None, 1, 1, None, 1, 1, 1, 1, 8, 0, 0.5, 0.4, 0.0, None, None, 0, 0.25, 2.0, 0.11, 0,
                                 None, None, None, None, 0, None) == -1
    assert N.lib.ssdk_map_match(None, None, None, 1, 4, None, 1, 3, 0.1, 0.5, None, None, None, None) == -1
    assert N.lib.ssdk_map_average_precision(None, None, None, 3, None, None) == -1
    assert N.lib.ssdk_match_loss_workspace_bytes(0, 1, 1, 1) == 0


def test_prototypes_derived_from_the_header_are_the_hand_written_ones():
    """ssds/_native.py reads argtypes / restype from include/ssdk.h.  These literals are the hand-written table that the
    derived binding replaced, for entry points that between them use every rule of the type map: size_t between ints,
    doubles and `void* const*`, a context with a descriptor pointer and floats, the longest list, no arguments at all, a
    pointer and a void return, a string return.  Host pointers (`int*`, `size_t*`, `char*`, `const float*`) are c_void_p like
    every pointer that is not a descriptor's: the header cannot tell them from device pointers."""
    from ssds import _native as N

    vp, i32, f32, f64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_size_t
    want = {
        "ssdk_pw_wgrad": ([vp, vp, vp, vp, sz, i32, i32, i32, i32, i32, vp], i32),
        "ssdk_adam_step": ([i32, vp, vp, vp, vp, vp, vp, vp, vp, f32, f64, f64, f32, f32, i32, vp, vp], i32),
        "ssdk_decode_nms_ctx": ([vp, ctypes.POINTER(N.Level), i32, i32, i32, f32, i32, i32, f32, i32, i32,
                                 vp, vp, vp, vp, vp, vp, vp, sz, vp], i32),
        "ssdk_device_info": ([vp, vp, vp, vp, i32], i32),
        "ssdk_neck_fuse_bwd": ([vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, i32, i32, vp, sz] + [i32] * 11 + [vp], i32),
        "ssdk_augment": ([vp, sz, ctypes.POINTER(N.AugmentDesc), i32, i32, i32, vp, vp, vp, i32, vp, sz, vp], i32),
        "ssdk_run_ops_ctx": ([vp, ctypes.POINTER(N.Op), i32, vp, sz, vp], i32),
        "ssdk_last_error": ([], ctypes.c_char_p),
        "ssdk_ctx_create": ([], vp),
        "ssdk_ctx_destroy": ([vp], None),
        "ssdk_conv_workspace_bytes": ([i32] * 8, sz),
        "ssdk_mbse_desc_bytes": ([], sz),
    }
    for name, (argtypes, restype) in want.items():
        fn = getattr(N.lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is restype, name
    # every declared entry point is bound, none left to ctypes' defaults
    assert len(N.EXPORTS) == 127
    for name in N.EXPORTS:
        assert getattr(N.lib, name).argtypes is not None, name


def test_header_parser_refuses_what_it_cannot_type():
    """A declaration outside the closed type map is an ImportError that quotes it -- never skipped, never defaulted to int."""
    from ssds import _native as N

    text = open(N.HEADER_PATH).read()
    head, tail = text.rsplit("#ifdef __cplusplus", 1)

    def with_decl(decl):
        return head + decl + "\n#ifdef __cplusplus" + tail

    today = N.parse_header(text)
    assert tuple(today.functions) == N.EXPORTS and today.constants["SSDK_VERSION"] == N.ABI_VERSION
    more = N.parse_header(with_decl("int ssdk_new_entry(const ssdk_conv_desc* desc, long long* keys, void* stream);"))
    assert more.functions["ssdk_new_entry"] == (ctypes.c_int, [ctypes.POINTER(more.structs["ssdk_conv_desc"]), ctypes.c_void_p,
                                                               ctypes.c_void_p])
    with pytest.raises(ImportError, match=r"unsigned flags.*int ssdk_new_entry\(const void\* x, unsigned flags, void\* stream\)"):
        N.parse_header(with_decl("int ssdk_new_entry(const void* x,\n    unsigned flags, void* stream);"))
    # an array parameter is a pointer in C: typing it by its first word would pass 4 bytes where the ABI takes an address
    with pytest.raises(ImportError, match=r"float mean\[3\].*int ssdk_new_entry\(const float mean\[3\], void\* stream\)"):
        N.parse_header(with_decl("int ssdk_new_entry(const float mean[3], void* stream);"))
    with pytest.raises(ImportError, match=r"int n\[\]"):
        N.parse_header(with_decl("int ssdk_new_entry(int n[]);"))
    with pytest.raises(ImportError, match=r"#define SSDK_NEW_FLAG \(1 << 3\)"):
        N.parse_header(with_decl("#define SSDK_NEW_FLAG (1 << 3)"))
    with pytest.raises(ImportError, match=r"float ssdk_new_entry\(int n\)"):
        N.parse_header(with_decl("float ssdk_new_entry(int n);"))
    with pytest.raises(ImportError, match=r"uint16_t flags.*typedef struct ssdk_new_desc"):
        N.parse_header(with_decl("typedef struct ssdk_new_desc {\n  const void* x;\n  uint16_t flags;\n} ssdk_new_desc;"))
    with pytest.raises(ImportError, match=r"SSDK_MAX_NOTHING"):
        N.parse_header(with_decl("typedef struct ssdk_new_desc { float v[SSDK_MAX_NOTHING * 4]; } ssdk_new_desc;"))


def test_import_without_library_or_header_says_which(tmp_path):
    """The module's source in another tree.  Without the library that is what is reported, with how to build it, whether the
    header is absent or cannot be parsed (no header error masks it); with a library file in place the header's own error
    shows: the declaration it cannot type, or the path at which it is missing."""
    import importlib.util

    from ssds import _native as N

    pkg = tmp_path / "ssds.pytorch_amd" / "ssds"
    pkg.mkdir(parents=True)
    (pkg / "_native.py").write_text(open(N.__file__).read())

    def load():
        spec = importlib.util.spec_from_file_location("_native_elsewhere", str(pkg / "_native.py"))
        spec.loader.exec_module(importlib.util.module_from_spec(spec))

    with pytest.raises(ImportError, match="libssdk.so not found at .* build it first"):
        load()
    (tmp_path / "include").mkdir()
    (tmp_path / "include" / "ssdk.h").write_text("#define SSDK_VERSION 245\nint ssdk_version(unsigned which);\n")
    with pytest.raises(ImportError, match="libssdk.so not found at .* build it first"):
        load()
    (tmp_path / "ssds.pytorch_amd" / "csrc").mkdir()
    (tmp_path / "ssds.pytorch_amd" / "csrc" / "libssdk.so").write_bytes(b"")
    with pytest.raises(ImportError, match=r"include/ssdk.h: .*unsigned which"):
        load()
    (tmp_path / "include" / "ssdk.h").unlink()
    with pytest.raises(ImportError, match="include/ssdk.h not found at " + re.escape(str(tmp_path / "include" / "ssdk.h"))):
        load()
