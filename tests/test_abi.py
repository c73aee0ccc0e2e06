"""CPU-side checks of the boundary: the HIP library builds for gfx950, loads, and exports every
symbol include/wsa.h declares.  No compute calls (no GPU here)."""
import os
import re

from webspeechanalyzer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_builds_and_exports_header_symbols():
    capi.build_library()
    L = capi.lib()
    assert L.wsa_abi_version() == capi.ABI_VERSION == 5
    header = open(os.path.join(ROOT, "include", "wsa.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(wsa_[a-z_0-9]+)\s*\(", header)))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/wsa.h but not exported by libwsa.so"
    assert sorted(capi.ABI_SYMBOLS) == declared


def _header_prototypes():
    """{name: (result, [parameter, ...])} of every function include/wsa.h declares, as C text without the parameter names' meaning:
    comments, preprocessor lines and the bodies of structs and enums are dropped first, so a prototype may span lines."""
    text = open(os.path.join(ROOT, "include", "wsa.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", " ", text, flags=re.M)
    text = text.replace('extern "C" {', " ")
    while True:
        text, n = re.subn(r"\{[^{}]*\}", " ", text)
        if not n:
            break
    protos = {}
    for stmt in text.split(";"):
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(wsa_\w+)\s*\(([^()]*)\)\s*", stmt)
        if not m or m.group(1).split()[0] == "typedef":
            continue
        params = [" ".join(p.split()) for p in m.group(3).split(",")]
        assert m.group(2) not in protos, m.group(2)
        protos[m.group(2)] = (" ".join(m.group(1).split()), [] if params == ["void"] else params)
    return protos


def _is_pointer_type(t):
    import ctypes
    return t is ctypes.c_void_p or t is ctypes.c_char_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def test_signature_table_matches_the_header():
    """capi.ABI_TABLE against the prototypes of include/wsa.h: the same functions, as many argtypes as parameters, every parameter and every
    result of the header's kind (a pointer for `*` and `[`, else the C type's own ctypes type; void is None).  The table alone is checked:
    capi.lib() applies it as it stands."""
    import ctypes
    scalar = {"double": ctypes.c_double, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int32_t": ctypes.c_int32, "int": ctypes.c_int32}
    result = {"wsa_status": ctypes.c_int, "int": ctypes.c_int, "void": None, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
              "int32_t": ctypes.c_int32}
    protos = _header_prototypes()
    assert len(protos) == 158
    assert sorted(protos) == sorted(capi.ABI_TABLE)
    assert any("[" in p for _, params in protos.values() for p in params), "no array parameter (`float out[4]`) parsed"
    for name, (res, params) in protos.items():
        restype, argtypes = capi.ABI_TABLE[name]
        assert len(argtypes) == len(params), f"{name}: {len(argtypes)} argtypes, {len(params)} parameters"
        for i, (p, t) in enumerate(zip(params, argtypes)):
            if "*" in p or "[" in p:
                assert _is_pointer_type(t), f"{name} parameter {i} ({p}): {t} is no pointer type"
            else:
                c_type = " ".join(w for w in p.split()[:-1] if w != "const")
                assert c_type in scalar, f"{name} parameter {i} ({p}): a C type this test does not know"
                assert t is scalar[c_type], f"{name} parameter {i} ({p}): {t}"
        if "*" in res:
            assert _is_pointer_type(restype), f"{name} returns {res}: {restype} is no pointer type"
        else:
            c_type = " ".join(w for w in res.split() if w != "const")
            assert c_type in result, f"{name} returns {res}: a C type this test does not know"
            assert restype is result[c_type], f"{name} returns {res}: {restype}"


def test_config_defaults_are_the_reference_defaults():
    c = capi.Config()
    # ref dist/main.js:2 @B2965
    assert (c["spec_type"], c["output_level"], c["f_min"], c["f_max"], c["N_fft_bins"], c["N_mel_bins"]) == (1, 4, 50, 4000, 256, 128)
    assert (c["window_width"], c["window_step"], c["pause_length"], c["min_seg_length"]) == (25, 25, 200, 50)
    assert (c["auto_noise_gate"], c["voiced_max_dB"], c["voiced_min_dB"], c["pre_norm_gain"], c["high_f_emph"]) == (1, 100, 10, 1000, 0)


def test_no_device_fails_loudly():
    import ctypes
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(capi.WsaError):
        capi.Analyzer(capi.Config())


def test_front_end_asm_blocks_are_the_generators_output():
    """csrc/fe_blocks.inc is generated (tools/gen/fe_blocks.py: operation lists -> register allocation -> asm text, every block replayed on
    random fp32 values against the plain formulas); the committed file must be what the generator prints."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "gen", "fe_blocks.py")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout == open(os.path.join(root, "webspeechanalyzer_amd", "csrc", "fe_blocks.inc")).read()
