"""CPU tier: the C-ABI library builds for gfx950, loads, exports every symbol include/sqd_hip.h
declares, and the ctypes signatures agree with the header (argument counts and kinds).
No compute call is made (there is no GPU in the build container)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_protos():
    txt = open(os.path.join(ROOT, "include", "sqd_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {}
    for m in re.finditer(r"\bint\s+(sqd_\w+)\s*\(([^)]*)\)\s*;", txt):
        args = [a.strip() for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
        protos[m.group(1)] = args
    return protos


def _kind(carg):
    if "*" in carg:
        return "ptr"
    if carg.startswith("float"):
        return "float"
    if carg.startswith("long long"):
        return "longlong"
    return "int"


def test_library_builds_and_exports_header_symbols():
    import __graft_entry__ as ge
    ge.build()
    from squeezedet_pytorch_amd import _native as nat
    lib = nat.lib()
    protos = _header_protos()
    assert len(protos) >= 14
    for name in protos:
        assert hasattr(lib, name), f"{name} declared in include/sqd_hip.h but not exported"


def test_ctypes_signatures_match_header():
    from squeezedet_pytorch_amd import _native as nat
    protos = _header_protos()
    sigs = dict(nat._SIGNATURES)
    sigs.update({k: v for k, v in nat._OPTIONAL.items() if k in protos})
    for name, cargs in protos.items():
        assert name in sigs, f"{name} has no ctypes signature"
        at = sigs[name]
        assert len(at) == len(cargs), f"{name}: header has {len(cargs)} args, ctypes {len(at)}"
        for c, t in zip(cargs, at):
            k = _kind(c)
            if k == "ptr":
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, c, t)
            elif k == "float":
                assert t is ctypes.c_float, (name, c, t)
            elif k == "longlong":
                assert t is ctypes.c_longlong, (name, c, t)
            else:
                assert t is ctypes.c_int, (name, c, t)


def test_status_codes_without_gpu():
    """Argument validation happens on the host before any launch, so it can be exercised here."""
    from squeezedet_pytorch_amd import _native as nat
    lib = nat.lib()
    n = lib.sqd_conv_num_cfgs()
    assert n >= 10
    t, k, px, bn = (ctypes.c_int() for _ in range(4))
    assert lib.sqd_conv_cfg_info(0, ctypes.byref(t), ctypes.byref(k), ctypes.byref(px), ctypes.byref(bn)) == 0
    assert t.value in (1, 9) and k.value in (16, 32, 64) and px.value in (64, 128, 256) and bn.value % 16 == 0
    assert lib.sqd_conv_cfg_is_dma(0) == 0 and lib.sqd_conv_cfg_is_dma(n) == -1
    assert lib.sqd_conv_cfg_info(n, None, None, None, None) == 1           # bad cfg id
    null = ctypes.c_void_p(0)
    assert lib.sqd_conv_fwd(null, null, null, null, null, null, null, 1, 1, 1, 4, 4, 0, 4, 16, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, null) == 1
    assert lib.sqd_detect_fwd(null, null, null, null, null, null, null, null, null, 1, 1, 3, 1, 1, 64, 0.4, 0.3, null) == 1


def test_wgrad_tile_form_without_gpu():
    """sqd_wgrad_tile_form is declared, bound and answers on the host: a form for each entry point (kind 0 = sqd_conv_wgrad,
    1 = sqd_conv_wgrad_group, 2 = sqd_squeeze_bwd), NULL outputs allowed, status codes for what the entries refuse."""
    from squeezedet_pytorch_amd import _native as nat
    assert 'sqd_wgrad_tile_form' in _header_protos() and 'sqd_wgrad_tile_form' in nat._SIGNATURES
    lib = nat.lib()

    def form(kind, taps, N, C):
        tn, tc, px = (ctypes.c_int(-1) for _ in range(3))
        rc = lib.sqd_wgrad_tile_form(kind, taps, N, C, ctypes.byref(tn), ctypes.byref(tc), ctypes.byref(px))
        return rc, (tn.value, tc.value, px.value)
    assert form(0, 1, 384, 512) == (0, (4, 8, 32))           # launch_wgrad<1, 4, 8, 2>
    assert form(0, 1, 16, 16) == (0, (1, 1, 128))            # launch_wgrad<1, 1, 1, 8>
    assert form(0, 1, 96, 64) == (0, (6, 4, 32))             # one 6-tile group
    assert form(0, 9, 72, 768) == (0, (5, 1, 64))            # ConvDet
    assert form(0, 9, 64, 64) == (0, (4, 2, 64))
    assert form(0, 9, 64, 48) == (0, (4, 1, 64))
    assert form(1, 1, 64, 16) == (0, (4, 1, 64))             # launch_wgrad_group<4, 1, 4>
    assert form(1, 1, 256, 384) == (0, (4, 8, 32))
    assert form(2, 1, 128, 64) == (0, (8, 4, 32))            # launch_wgrad<1, 8, 4, 2, true>
    assert form(2, 1, 16, 96) == (0, (1, 4, 32))
    assert lib.sqd_wgrad_tile_form(0, 1, 64, 64, None, None, None) == 0
    for bad in ((3, 1, 64, 64), (-1, 1, 64, 64), (0, 3, 64, 64), (0, 1, 0, 64), (0, 1, 64, 0)):
        assert form(*bad) == (nat.ERR_BAD_ARG, (-1, -1, -1)), bad
    for refused in ((1, 1, 48, 64), (1, 1, 96, 64), (1, 9, 64, 64), (2, 1, 132, 64), (2, 9, 64, 64)):
        assert form(*refused) == (nat.ERR_UNSUPPORTED, (-1, -1, -1)), refused


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from squeezedet_pytorch_amd import _native as nat
    monkeypatch.setattr(nat, "_lib", None)
    monkeypatch.setattr(nat, "_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(nat.NativeLibraryError):
        nat.lib()
