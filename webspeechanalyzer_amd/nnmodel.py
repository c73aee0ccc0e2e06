"""The reference application's trained classifiers (dist/nnmodel/<db>/cats_<label>/ — model.json, model_meta.json,
model.weights.bin as ml5 0.6.0 saves them) parsed into what wsa_model_create takes, and its regression models (ords_<label>/: one
output unit, no legend, the output range in model_meta.json's outputs.y.{min,max}).  Pure Python: no device needed."""
import json
import os

import numpy as np

NFEAT = 53
# the row width of every output level whose ML panel the app enables (ref src/index.js:723, src/localstore.js:7 process_exp_features_len;
# wsa_level_feature_count of include/wsa.h): a model's input count is one of these
LEVEL_FEATURES = {5: 53, 11: 264, 12: 23, 13: 53}
WIDTHS = (53, 264, 23)
WIDTHS_TEXT = "53 (output_level 5 and 13), 264 (output_level 11) or 23 (output_level 12)"
ACT = {"linear": 0, "relu": 1, "sigmoid": 2, "tanh": 3, "softmax": 4}
MAX_LAYERS, MAX_WIDTH, MAX_CLASSES = 8, 1024, 64


class ModelFormatError(ValueError):
    pass


class ModelSpec:
    """units [n_layers + 1], activation names, kernels [in][out] f32, biases f32, in_min / in_max f64, labels (legend order).
    A regression model has out_min / out_max (the range its one output is un-normalised with) and no labels."""

    def __init__(self, units, activations, kernels, biases, in_min, in_max, labels, out_min=None, out_max=None):
        self.units, self.activations, self.kernels, self.biases = units, activations, kernels, biases
        self.in_min, self.in_max, self.labels = in_min, in_max, labels
        self.out_min, self.out_max = out_min, out_max

    @property
    def is_regression(self):
        return self.out_min is not None and self.out_max is not None

    @property
    def n_classes(self):
        return self.units[-1]


def parse(model_json, meta_json, weights):
    """model_json / meta_json: dicts or JSON text; weights: the bytes of model.weights.bin.  Raises ModelFormatError."""
    mj = json.loads(model_json) if isinstance(model_json, (str, bytes)) else model_json
    meta = json.loads(meta_json) if isinstance(meta_json, (str, bytes)) else meta_json
    try:
        topo = mj["modelTopology"]
        layers = topo["config"]["layers"] if isinstance(topo["config"], dict) else topo["config"]
        manifest = [w for group in mj["weightsManifest"] for w in group["weights"]]
    except (KeyError, TypeError) as e:
        raise ModelFormatError(f"model.json: no modelTopology / weightsManifest ({e})")
    if topo.get("class_name") != "Sequential":
        raise ModelFormatError(f"model.json: a {topo.get('class_name')} model; only Sequential stacks of Dense layers are supported")
    if not 1 <= len(layers) <= MAX_LAYERS:
        raise ModelFormatError(f"model.json: {len(layers)} layers (1 .. {MAX_LAYERS} supported)")
    acts = []
    for i, l in enumerate(layers):
        if l.get("class_name") != "Dense":
            raise ModelFormatError(f"model.json: layer {i} is {l.get('class_name')}; only Dense layers are supported")
        a = l["config"].get("activation", "linear")
        if a not in ACT:
            raise ModelFormatError(f"model.json: layer {i} has activation {a!r}")
        if a == "softmax" and i != len(layers) - 1:
            raise ModelFormatError("model.json: softmax is only supported on the last layer")
        if not l["config"].get("use_bias", True):
            raise ModelFormatError(f"model.json: layer {i} has no bias")
        acts.append(a)
    if len(manifest) != 2 * len(layers):
        raise ModelFormatError(f"weightsManifest lists {len(manifest)} tensors for {len(layers)} Dense layers (kernel + bias each)")
    total = 0
    for w in manifest:
        if w.get("dtype", "float32") != "float32":
            raise ModelFormatError(f"weight {w.get('name')}: dtype {w.get('dtype')} (float32 only)")
        total += int(np.prod(w["shape"])) * 4
    weights = bytes(weights)
    if len(weights) != total:
        raise ModelFormatError(f"model.weights.bin holds {len(weights)} bytes, the weightsManifest needs {total}")
    units = [int(manifest[0]["shape"][0])]
    kernels, biases, off = [], [], 0
    for i in range(len(layers)):
        ks, bs = manifest[2 * i]["shape"], manifest[2 * i + 1]["shape"]
        if len(ks) != 2 or ks[0] != units[-1] or bs != [ks[1]] or ks[1] != layers[i]["config"]["units"]:
            raise ModelFormatError(f"layer {i}: kernel {ks} / bias {bs} do not chain from {units[-1]} inputs to {layers[i]['config']['units']} units")
        k = np.frombuffer(weights, "<f4", ks[0] * ks[1], off).reshape(ks).copy(); off += k.nbytes
        b = np.frombuffer(weights, "<f4", bs[0], off).copy(); off += b.nbytes
        kernels.append(k); biases.append(b); units.append(int(ks[1]))
    if units[0] not in WIDTHS:
        raise ModelFormatError(f"the model takes {units[0]} inputs; the feature rows have {WIDTHS_TEXT}")
    if max(units[1:]) > MAX_WIDTH or units[-1] > MAX_CLASSES:
        raise ModelFormatError(f"layer widths {units[1:]} exceed {MAX_WIDTH} (or more than {MAX_CLASSES} outputs)")
    try:
        ins = meta["inputs"]
        in_min = np.array([float(ins[str(i)]["min"]) for i in range(units[0])])
        in_max = np.array([float(ins[str(i)]["max"]) for i in range(units[0])])
        y = meta["outputs"].get("y") if isinstance(meta["outputs"], dict) else None
        regression = isinstance(y, dict) and "legend" not in y and "min" in y and "max" in y
        if regression:
            out_min, out_max = float(y["min"]), float(y["max"])
    except (KeyError, TypeError, ValueError) as e:
        raise ModelFormatError(f"model_meta.json: no inputs '0'..'{units[0] - 1}' min / max or output legend ({e})")
    if regression:                                   # ml5 task "regression": outputs.y = {dtype: "number", min, max}
        if not (np.all(np.isfinite(in_min)) and np.all(np.isfinite(in_max))):
            raise ModelFormatError("model_meta.json: non-finite input range")
        if units[-1] != 1 or acts[-1] == "softmax":
            raise ModelFormatError(f"model_meta.json describes a regression output; the model ends in {units[-1]} {acts[-1]} units")
        if not (np.isfinite(out_min) and np.isfinite(out_max)) or out_max == out_min:
            raise ModelFormatError(f"model_meta.json: output range {out_min} .. {out_max}")
        return ModelSpec(units, acts, kernels, biases, in_min, in_max, [], out_min, out_max)
    try:
        legend = list(meta["outputs"]["y"]["legend"].keys()) if "y" in meta["outputs"] else list(next(iter(meta["outputs"].values()))["legend"].keys())
    except (KeyError, TypeError, StopIteration) as e:
        raise ModelFormatError(f"model_meta.json: no inputs '0'..'{units[0] - 1}' min / max or output legend ({e})")
    if not (np.all(np.isfinite(in_min)) and np.all(np.isfinite(in_max))):
        raise ModelFormatError("model_meta.json: non-finite input range")
    if acts[-1] == "softmax" and len(legend) != units[-1]:
        raise ModelFormatError(f"model_meta.json: {len(legend)} legend labels for {units[-1]} outputs")
    return ModelSpec(units, acts, kernels, biases, in_min, in_max, legend)


def load_dir(path):
    """A directory as the app ships it: model.json, model_meta.json, model.weights.bin (the manifest's path)."""
    with open(os.path.join(path, "model.json")) as f:
        mj = json.load(f)
    with open(os.path.join(path, "model_meta.json")) as f:
        meta = json.load(f)
    paths = [p for g in mj.get("weightsManifest", []) for p in g.get("paths", [])] or ["model.weights.bin"]
    data = b"".join(open(os.path.join(path, os.path.basename(p)), "rb").read() for p in paths)
    return parse(mj, meta, data)


def save_dir(spec, path):
    """Writes model.json, model_meta.json and model.weights.bin as ml5 0.6.0's neuralNetwork.save does (download_nn_model of
    src/neuralmodel.js), in the key layout of the directories the app ships: load_dir reads them back bit for bit, and ml5's
    neuralNetwork.load takes them."""
    nl = len(spec.kernels)
    if len(spec.in_min) != spec.units[0] or len(spec.in_max) != spec.units[0]:
        raise ModelFormatError(f"the model takes {spec.units[0]} inputs; in_min / in_max hold {len(spec.in_min)} / {len(spec.in_max)} ranges")
    regression = getattr(spec, "is_regression", False)
    if regression and (spec.units[-1] != 1 or spec.activations[-1] == "softmax"):
        raise ModelFormatError(f"a regression model ends in one non-softmax unit, not {spec.units[-1]} {spec.activations[-1]}")
    if not regression and len(spec.labels) != spec.units[-1]:
        raise ModelFormatError(f"{len(spec.labels)} legend labels for {spec.units[-1]} outputs")
    layers, weights, blob = [], [], []
    for i in range(nl):
        name = f"dense_Dense{i + 1}"
        cfg = {"units": int(spec.units[i + 1]), "activation": spec.activations[i], "use_bias": True,
               "kernel_initializer": {"class_name": "VarianceScaling", "config": {"scale": 1, "mode": "fan_avg", "distribution": "normal", "seed": None}},
               "bias_initializer": {"class_name": "Zeros", "config": {}},
               "kernel_regularizer": None, "bias_regularizer": None, "activity_regularizer": None, "kernel_constraint": None, "bias_constraint": None,
               "name": name, "trainable": True}
        if i == 0:
            cfg.update(batch_input_shape=[None, int(spec.units[0])], dtype="float32")
        layers.append({"class_name": "Dense", "config": cfg})
        k = np.ascontiguousarray(spec.kernels[i], "<f4")
        b = np.ascontiguousarray(spec.biases[i], "<f4")
        if k.shape != (spec.units[i], spec.units[i + 1]) or b.shape != (spec.units[i + 1],):
            raise ModelFormatError(f"layer {i}: kernel {k.shape} / bias {b.shape} do not match units {spec.units}")
        weights += [{"name": name + "/kernel", "shape": list(k.shape), "dtype": "float32"}, {"name": name + "/bias", "shape": list(b.shape), "dtype": "float32"}]
        blob += [k.tobytes(), b.tobytes()]
    mj = {"modelTopology": {"class_name": "Sequential", "config": {"name": "sequential_1", "layers": layers},
                            "keras_version": "tfjs-layers 1.7.2", "backend": "tensor_flow.js"},
          "weightsManifest": [{"paths": ["./model.weights.bin"], "weights": weights}]}
    labels = [str(x) for x in spec.labels]
    C = len(labels)
    meta = {"inputUnits": [int(spec.units[0])], "outputUnits": C,
            "inputs": {str(i): {"dtype": "number", "min": float(spec.in_min[i]), "max": float(spec.in_max[i])} for i in range(int(spec.units[0]))},
            "outputs": {"y": {"dtype": "string", "min": 0, "max": 1, "uniqueValues": labels,
                              "legend": {lab: [1 if c == j else 0 for c in range(C)] for j, lab in enumerate(labels)}}},
            "isNormalized": True}
    if regression:                                   # as ml5 writes a task "regression" model: no legend, the output's range
        meta["outputUnits"] = 1
        meta["outputs"] = {"y": {"dtype": "number", "min": float(spec.out_min), "max": float(spec.out_max)}}
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "model.json"), "w") as f:
        json.dump(mj, f)
    with open(os.path.join(path, "model_meta.json"), "w") as f:
        json.dump(meta, f)
    with open(os.path.join(path, "model.weights.bin"), "wb") as f:
        f.write(b"".join(blob))
