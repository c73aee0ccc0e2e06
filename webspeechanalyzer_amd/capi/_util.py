"""What the binding's classes share: the life of a library handle and the copy of a host table the library hands out."""
import ctypes
import functools

import numpy as np


class _Handle:
    """An object of the library behind `h`.  A subclass sets `L` and creates `h` in its __init__ and names the function that destroys it."""
    _destroy = None            # e.g. "wsa_model_destroy"
    h = None                   # a c_void_p; null before the object is created and after close()

    def close(self):
        if self.h:
            getattr(self.L, self._destroy)(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@functools.lru_cache(maxsize=None)
def _pointer_type(dtype):
    return ctypes.POINTER(np.ctypeslib.as_ctypes_type(dtype))


def host_copy(ptr, dtype, shape, null_is_none=False):
    """An owned array of `shape` and `dtype` copied from the host memory at `ptr` (an address as a c_void_p field gives it).  An empty
    shape reads nothing.  null_is_none: a null `ptr` gives None, whatever the shape (a table the library does not hand out at this
    level); without it the caller knows the pointer is set, and it is not looked at."""
    if null_is_none and not ptr:
        return None
    if not int(np.prod(shape)):
        return np.zeros(shape, dtype)
    return np.ctypeslib.as_array(ctypes.cast(ptr, _pointer_type(dtype)), shape=shape).copy()
