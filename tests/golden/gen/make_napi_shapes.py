"""Records tests/golden/napi_shapes.json from a built addon (needs a GPU; tests/test_gpu_napi_shapes.py says what is recorded).
usage: python tests/golden/gen/make_napi_shapes.py path/to/wsa_napi.node [out.json]
The addon must lie beside a libwsa.so.  Refuses to write a golden in which some recorded object has no rows: choose another seed then."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from tests import test_gpu_napi_shapes as T  # noqa: E402


def main():
    addon = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
    with tempfile.TemporaryDirectory() as tmp:
        got = T.record(addon, tmp)
    with open(out, "w") as f:
        # one line per result object, so that a changed shape shows as one changed line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(got[k], sort_keys=True)}" for k in sorted(got)) + "\n}\n")
    print(f"{len(got)} objects -> {out}")
    for name, shape in got.items():
        n = T.rows_of(name, shape)
        print(f"{name}: {n} rows")
        if n <= 0:
            sys.exit(f"{name} has no rows: an empty table proves nothing about its writer; do not commit {out}")


if __name__ == "__main__":
    main()
