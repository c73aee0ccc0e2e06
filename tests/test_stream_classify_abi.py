"""CPU-side checks of the stream classifier's boundary: libwsa.so exports wsa_stream_set_model / wsa_stream_classes, and NULL
arguments are refused with WSA_ERR_INVALID before anything touches a device."""
import ctypes

from webspeechanalyzer_amd import capi

WSA_ERR_INVALID = 1


def test_stream_classifier_symbols_are_exported_and_refuse_null():
    capi.build_library()
    L = capi.lib()
    for name in ("wsa_stream_set_model", "wsa_stream_classes"):
        assert hasattr(L, name) and name in capi.ABI_SYMBOLS
    assert L.wsa_stream_set_model(None, None) == WSA_ERR_INVALID
    assert L.wsa_stream_classes(None, None) == WSA_ERR_INVALID
    r = capi._StreamClassResult()
    assert L.wsa_stream_classes(None, ctypes.byref(r)) == WSA_ERR_INVALID
    assert (r.n_rows, r.n_callbacks, r.prob) == (0, 0, None)
    assert ctypes.sizeof(capi._StreamClassResult) == 4 * 4 + 5 * ctypes.sizeof(ctypes.c_void_p)
