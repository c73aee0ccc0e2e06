"""ctypes binding of include/wsa.h (libwsa.so).  No CPU fallback: if the HIP library is missing or no
gfx950 device is present, construction raises.

One module per job; everything is imported from here (`from webspeechanalyzer_amd import capi`):
_abi the structures, constants, signatures and the loader, _util the handle base and the host copy, pcm, analyzer, batch, streams,
models, training, db, gather the product's objects, debug the wsa_debug_* test entries."""
from ._abi import *  # noqa: F401,F403
from ._abi import (_BatchInfo, _ClassResult, _Config, _DeviceResult, _EnsembleHost, _EnsembleResult, _Geometry, _HERE, _KnnFoldResult,  # noqa: F401
                   _KnnResult, _ModelDesc, _PCM_DTYPE, _PCM_ELEMS, _PCM_NAMES, _StreamClassResult, _StreamDbResult, _StreamEnsembleResult,
                   _StreamKnnResult, _StreamRows, _StreamValueResult, _TrainStats, _U32x8, _ValueHost, _ValueResult, _VP8, _VPH)
from .pcm import *  # noqa: F401,F403
from .pcm import _pcm_array  # noqa: F401
from .batch import *  # noqa: F401,F403
from .batch import _track_records  # noqa: F401
from .streams import *  # noqa: F401,F403
from .models import *  # noqa: F401,F403
from .models import _model_desc  # noqa: F401
from .training import *  # noqa: F401,F403
from .db import *  # noqa: F401,F403
from .db import _DB_AGREE, _DB_CAT, _DB_CLASS, _DB_ORD  # noqa: F401
from .gather import *  # noqa: F401,F403
from .gather import _GatherResult  # noqa: F401
from .analyzer import *  # noqa: F401,F403
from .debug import *  # noqa: F401,F403
from .debug import _DebugClassifyIO, _DebugCompactIO, _DebugFoldIO  # noqa: F401
