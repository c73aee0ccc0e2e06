"""PCM formats and channel selection (specs PK-1 .. PK-3) and the pure host entries."""
import numpy as np

from ._abi import CHANNEL_MIX, WsaError, _PCM_DTYPE, _PCM_ELEMS, _PCM_NAMES, lib


def pcm_format(fmt):
    """A WSA_PCM_* number from a number or one of 'f32', 'i16', 'mulaw', 'alaw', 'u8', 'i24', 'i32', 'f64'; anything else is refused."""
    if isinstance(fmt, str):
        if fmt not in _PCM_NAMES:
            raise WsaError(f"unknown input format {fmt!r} ('f32', 'i16', 'mulaw', 'alaw', 'u8', 'i24', 'i32', 'f64')")
        return _PCM_NAMES[fmt]
    if isinstance(fmt, (bool, float)) or int(fmt) not in _PCM_DTYPE:
        raise WsaError(f"unknown input format {fmt!r} (PCM_F32 0, PCM_I16 1, PCM_MULAW 2, PCM_ALAW 3, PCM_U8 8, PCM_I24 9, PCM_I32 10, PCM_F64 11)")
    return int(fmt)


def _pcm_array(fmt, f, array):
    """`array` as the contiguous flat samples of format `f`; the wrong sample type is refused, never converted."""
    a = np.ascontiguousarray(array)
    if a.dtype != _PCM_DTYPE[f]:
        raise WsaError(f"format {fmt!r} takes {np.dtype(_PCM_DTYPE[f]).name} samples, not {a.dtype.name}")
    return a.reshape(-1)


def channel_select(select, channels=None):
    """A PK-3 `select` word from a channel index or 'mix' (or CHANNEL_MIX); with `channels` given, an index at or above it is refused."""
    if isinstance(select, str):
        if select != "mix":
            raise WsaError(f"select {select!r}: a channel index or 'mix'")
        return CHANNEL_MIX
    if isinstance(select, (bool, float)) or not 0 <= int(select) <= CHANNEL_MIX:
        raise WsaError(f"select {select!r}: a channel index or 'mix'")
    s = int(select)
    if channels is not None and s != CHANNEL_MIX and s >= int(channels):
        raise WsaError(f"select {s} is neither a channel below {int(channels)} nor 'mix'")
    return s


def pcm_decode(fmt, array, channels=1, select=0):
    """Specs PK-1 / PK-2 / PK-3 on the host (wsa_pcm_decode_select, no device): channel `select` (0 by default; 'mix': the mono mix) of the
    interleaved frames in `array` (int16 for 'i16', uint8 for the G.711 laws and 'u8', three uint8 per sample for 'i24', int32 for 'i32',
    float64 for 'f64', float32 for 'f32'; a trailing partial frame is ignored where it does not hold the selected channel) as float32 — the
    floats a stream set or a batch fed `array` analyses."""
    f = pcm_format(fmt)
    ch = int(channels)
    if not 1 <= ch <= 64:
        raise WsaError(f"channel count {ch} outside 1 .. 64")
    sel = channel_select(select, ch)
    a = _pcm_array(fmt, f, array)
    size = a.size // _PCM_ELEMS.get(f, 1)            # whole samples
    last = ch - 1 if sel == CHANNEL_MIX else sel     # the last channel of a frame that is read
    n = (size - 1 - last) // ch + 1 if size > last else 0          # frames whose selected channel (the mix: every channel) is present
    out = np.zeros(n, np.float32)
    if lib().wsa_pcm_decode_select(f, a.ctypes.data, n, ch, sel, out.ctypes.data) != 0:
        raise WsaError("wsa_pcm_decode_select refused its arguments")
    return out


def pcm_channels_tile_frames(fmt, channels):
    """wsa_pcm_channels_tile_frames: the frames of one source a workgroup of batch_deinterleave_kernel takes at a time (spec PK-3)."""
    return int(lib().wsa_pcm_channels_tile_frames(pcm_format(fmt), int(channels)))


def level_feature_count(output_level):
    """wsa_level_feature_count: 53 (levels 5 and 13), 264 (level 11), 23 (level 12), 0 at any other level."""
    return int(lib().wsa_level_feature_count(int(output_level)))
