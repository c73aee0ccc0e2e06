// trainmodel.js — the host side of training the app's classifiers (specification TR-1, K7): what src/neuralmodel.js:163-403 (train_nn) does
// around ml5.neuralNetwork(...).train — selecting and balancing the stored rows, the input ranges — plus what the reference draws from
// Math.random and TR-1 leaves to the host (initial weights, one order of the training rows per epoch; here from a seeded generator of our own),
// and the three files ml5 0.6.0's save() writes.  Pure JavaScript, no device.  Classification only; the '*' wildcard class is not supported.
// (prepare / stack; the regression models, specification TR-2, have prepareOrdinal / stackRegression below: ref neuralmodel.js:268-333.)
'use strict';
const fs = require('fs');
const path = require('path');

const ACT = { linear: 0, relu: 1, sigmoid: 2, tanh: 3, softmax: 4 };
const ACT_NAME = Object.keys(ACT);
const WIDTHS = [53, 264, 23];        // the row width of an ML level: 5 and 13, 11, 12 (ref src/localstore.js:7; wsa_level_feature_count)
// the width of the rows: that of the first one, which must be an ML level's; every row used is checked against it
function rowWidth(features, who) {
  const w = features.length && features[0] ? features[0].length : 0;
  if (WIDTHS.indexOf(w) < 0) throw who + ': row 0 has ' + w + ' features; 53 expected (or 264 at output_level 11, 23 at output_level 12)';
  return w;
}
const DEFAULT_OPTIONS = { layers: [{ type: 'dense', units: 8, activation: 'relu' }, { type: 'dense', activation: 'softmax' }], learningRate: 0.2 };   // ref src/neuralmodel_aux.js:106-124

// ref neuralmodel.js:216-264: rows whose label is one of `classes` in DB order; fewer than 10 refused; every class with more than 3 and fewer
// than the largest count is topped up by cycling through the DB in order; min / max over the balanced set; legend = order of first appearance
// the label-only half: which DB rows are added, in which order, with which class index (nothing here reads a feature, so it serves host rows and a device DB alike)
function select(labels, classes) {
  classes = classes.map(String);
  if (classes.indexOf('*') >= 0) throw "trainModel: the '*' wildcard class is not supported";
  const n = labels.length;
  const cls = labels.map((v) => (v === null || v === undefined ? -1 : classes.indexOf(String(v))));
  const rows = [], count = new Array(classes.length).fill(0);
  cls.forEach((c, i) => { if (c >= 0) { rows.push(i); count[c]++; } });
  if (rows.length < 10) throw 'Sample size ' + rows.length + '/' + n + ' too small for training';
  const max_n = Math.max(...count);
  for (let c = 0; c < classes.length; c++)
    while (count[c] < max_n && count[c] > 3)
      for (let i = 0; i < n; i++) {
        if (cls[i] === c && count[c] < max_n) { rows.push(i); count[c]++; }
        if (count[c] >= max_n) break;
      }
  const legend = [];
  for (const i of rows) if (legend.indexOf(classes[cls[i]]) < 0) legend.push(classes[cls[i]]);
  return { rows, y: Int32Array.from(rows, (i) => legend.indexOf(classes[cls[i]])), legend, counts: count };
}
function prepare(features, labels, classes) {
  if (classes.map(String).indexOf('*') >= 0) throw "trainModel: the '*' wildcard class is not supported";
  if (!Array.isArray(features) || features.length !== labels.length) throw 'trainModel: features and labels must have one entry per row';
  const { rows, y, legend, counts } = select(labels, classes);
  const W = rowWidth(features, 'trainModel');
  const x = new Float64Array(rows.length * W);
  const inMin = new Float64Array(W).fill(Infinity), inMax = new Float64Array(W).fill(-Infinity);
  rows.forEach((i, r) => {
    if (features[i].length !== W) throw 'trainModel: row ' + i + ' has ' + features[i].length + ' features; ' + W + ' expected';
    for (let k = 0; k < W; k++) { const v = Number(features[i][k]); x[r * W + k] = v; if (v < inMin[k]) inMin[k] = v; if (v > inMax[k]) inMax[k] = v; }
  });
  return { features: x, y, legend, inMin, inMax, counts, rows, width: W };
}

function rng(seed) {            // mulberry32: 32 bits of state, enough for weights and shuffles that only have to be repeatable
  let a = (seed >>> 0) || 1;
  return () => { a = (a + 0x6D2B79F5) >>> 0; let t = a; t = Math.imul(t ^ (t >>> 15), t | 1); t ^= t + Math.imul(t ^ (t >>> 7), t | 61); return ((t ^ (t >>> 14)) >>> 0) / 4294967296; };
}
// tfjs's default Dense initialisers: truncated normal (redrawn beyond two standard deviations), sd sqrt(2 / (fan_in + fan_out)); zero biases
function glorotInit(units, seed) {
  const u = rng(seed), kernels = [], biases = [];
  const normal = () => { let z; do { z = Math.sqrt(-2 * Math.log(1 - u())) * Math.cos(2 * Math.PI * u()); } while (Math.abs(z) > 2); return z; };
  for (let l = 0; l + 1 < units.length; l++) {
    const sd = Math.sqrt(2 / (units[l] + units[l + 1])), k = new Float32Array(units[l] * units[l + 1]);
    for (let i = 0; i < k.length; i++) k[i] = normal() * sd;
    kernels.push(k); biases.push(new Float32Array(units[l + 1]));
  }
  return { kernels, biases };
}
function epochOrders(nTrain, epochs, seed) {       // one Fisher-Yates permutation per epoch, [epochs][nTrain]
  const u = rng(seed), out = new Uint32Array(epochs * nTrain);
  for (let e = 0; e < epochs; e++) {
    const o = out.subarray(e * nTrain, (e + 1) * nTrain);
    for (let i = 0; i < nTrain; i++) o[i] = i;
    for (let i = nTrain - 1; i > 0; i--) { const j = Math.floor(u() * (i + 1)), t = o[i]; o[i] = o[j]; o[j] = t; }
  }
  return out;
}
// ref src/neuralmodel_aux.js:127-150 (nn_default_options_ords: task "regression")
const DEFAULT_OPTIONS_ORDS = { layers: [{ type: 'dense', units: 64, activation: 'sigmoid' }, { type: 'dense', units: 16, activation: 'sigmoid' }, { type: 'dense', activation: 'sigmoid' }], learningRate: 0.2 };
const ORDINAL_RANGES = [0.25, 0.5, 0.75, 1.0];
// ref neuralmodel.js:278-332: a row's bin is the first range that holds its value; null / undefined and values above 1.0 are dropped; fewer than 10
// rows refused; only when the largest bin exceeds 3, every bin with more than 3 and fewer than the largest count is topped up by cycling through
// the DB in order; the input and output ranges over the balanced set
function selectOrdinal(values) {
  const nb = ORDINAL_RANGES.length, n = values.length;
  const bins = values.map((v) => (v === null || v === undefined ? -1 : ORDINAL_RANGES.findIndex((hi) => v <= hi)));       // -1: above 1.0 (or NaN)
  const rows = [], count = new Array(nb).fill(0);
  bins.forEach((b, i) => { if (b >= 0) { rows.push(i); count[b]++; } });
  if (rows.length < 10) throw 'Sample size ' + rows.length + '/' + n + ' too small for training';
  const max_n = Math.max(...count);
  if (max_n > 3)
    for (let c = 0; c < nb; c++)
      while (count[c] < max_n && count[c] > 3)
        for (let i = 0; i < n; i++) {
          if (bins[i] === c && count[c] < max_n) { rows.push(i); count[c]++; }
          if (count[c] >= max_n) break;
        }
  const y = Float64Array.from(rows, (i) => Number(values[i]));
  let outMin = Infinity, outMax = -Infinity;
  for (const v of y) { if (v < outMin) outMin = v; if (v > outMax) outMax = v; }
  return { rows, values: y, outMin, outMax, counts: count };
}
function prepareOrdinal(features, values) {
  if (!Array.isArray(features) || features.length !== values.length) throw 'trainRegression: features and values must have one entry per row';
  const sel = selectOrdinal(values), rows = sel.rows;
  const W = rowWidth(features, 'trainRegression');
  const x = new Float64Array(rows.length * W);
  const inMin = new Float64Array(W).fill(Infinity), inMax = new Float64Array(W).fill(-Infinity);
  rows.forEach((i, r) => {
    if (features[i].length !== W) throw 'trainRegression: row ' + i + ' has ' + features[i].length + ' features; ' + W + ' expected';
    for (let k = 0; k < W; k++) { const v = Number(features[i][k]); x[r * W + k] = v; if (v < inMin[k]) inMin[k] = v; if (v > inMax[k]) inMax[k] = v; }
  });
  return { features: x, values: sel.values, inMin, inMax, outMin: sel.outMin, outMax: sel.outMax, counts: sel.counts, rows, width: W };
}
function stackRegression(layers, nInputs) {
  const units = [nInputs === undefined ? 53 : nInputs], activation = [];
  layers.forEach((l, i) => {
    if ((l.type || 'dense') !== 'dense') throw 'trainRegression: layer ' + i + ' is ' + l.type + '; only dense layers are supported';
    const a = l.activation || 'linear';
    if (!(a in ACT)) throw 'trainRegression: layer ' + i + ' has activation ' + a;
    units.push(i === layers.length - 1 ? 1 : l.units | 0); activation.push(ACT[a]);
  });
  if (activation[activation.length - 1] === ACT.softmax) throw "trainRegression: a regression model's last layer is linear, relu, sigmoid or tanh, not softmax";
  return { units: Int32Array.from(units), activation: Int32Array.from(activation) };
}
function split(n, validationSplit) { const nTrain = Math.floor(n * (1 - (validationSplit === undefined ? 0.1 : validationSplit))); return { nTrain, nVal: n - nTrain }; }
function stack(layers, nClasses, nInputs) {
  const units = [nInputs === undefined ? 53 : nInputs], activation = [];
  layers.forEach((l, i) => {
    if ((l.type || 'dense') !== 'dense') throw 'trainModel: layer ' + i + ' is ' + l.type + '; only dense layers are supported';
    const a = l.activation || 'linear';
    if (!(a in ACT)) throw 'trainModel: layer ' + i + ' has activation ' + a;
    units.push(i === layers.length - 1 ? nClasses : l.units | 0); activation.push(ACT[a]);
  });
  if (activation[activation.length - 1] !== ACT.softmax) throw 'trainModel: training needs a softmax output layer';
  return { units: Int32Array.from(units), activation: Int32Array.from(activation) };
}

// model.json, model_meta.json, model.weights.bin in the key layout of the directories the app ships (dist/nnmodel/<db>/cats_<label>/)
function saveModelFiles(spec, dir) {
  const nl = spec.kernels.length, layers = [], weights = [], blobs = [];
  const regression = typeof spec.outMin === 'number' && typeof spec.outMax === 'number';       // ords_<label>: no legend, the output's range
  if (regression && (spec.units[nl] !== 1 || spec.activation[nl - 1] === ACT.softmax)) throw 'saveModel: a regression model ends in one non-softmax unit';
  if (!regression && spec.labels.length !== spec.units[nl]) throw 'saveModel: ' + spec.labels.length + ' legend labels for ' + spec.units[nl] + ' outputs';
  for (let i = 0; i < nl; i++) {
    const name = 'dense_Dense' + (i + 1);
    const cfg = { units: spec.units[i + 1], activation: ACT_NAME[spec.activation[i]], use_bias: true,
      kernel_initializer: { class_name: 'VarianceScaling', config: { scale: 1, mode: 'fan_avg', distribution: 'normal', seed: null } },
      bias_initializer: { class_name: 'Zeros', config: {} }, kernel_regularizer: null, bias_regularizer: null, activity_regularizer: null,
      kernel_constraint: null, bias_constraint: null, name, trainable: true };
    if (i === 0) { cfg.batch_input_shape = [null, spec.units[0]]; cfg.dtype = 'float32'; }
    layers.push({ class_name: 'Dense', config: cfg });
    weights.push({ name: name + '/kernel', shape: [spec.units[i], spec.units[i + 1]], dtype: 'float32' }, { name: name + '/bias', shape: [spec.units[i + 1]], dtype: 'float32' });
    for (const a of [spec.kernels[i], spec.biases[i]]) blobs.push(Buffer.from(a.buffer, a.byteOffset, a.byteLength));
  }
  const mj = { modelTopology: { class_name: 'Sequential', config: { name: 'sequential_1', layers }, keras_version: 'tfjs-layers 1.7.2', backend: 'tensor_flow.js' },
    weightsManifest: [{ paths: ['./model.weights.bin'], weights }] };
  const inputs = {}, legend = {}, C = spec.labels.length;
  for (let k = 0; k < spec.units[0]; k++) inputs[String(k)] = { dtype: 'number', min: spec.inMin[k], max: spec.inMax[k] };
  spec.labels.forEach((lab, j) => { legend[lab] = Array.from({ length: C }, (_, c) => (c === j ? 1 : 0)); });
  const meta = { inputUnits: [spec.units[0]], outputUnits: C, inputs, outputs: { y: { dtype: 'string', min: 0, max: 1, uniqueValues: spec.labels.slice(), legend } }, isNormalized: true };
  if (regression) { meta.outputUnits = 1; meta.outputs = { y: { dtype: 'number', min: spec.outMin, max: spec.outMax } }; }
  fs.mkdirSync(dir, { recursive: true });
  fs.writeFileSync(path.join(dir, 'model.json'), JSON.stringify(mj));
  fs.writeFileSync(path.join(dir, 'model_meta.json'), JSON.stringify(meta));
  fs.writeFileSync(path.join(dir, 'model.weights.bin'), Buffer.concat(blobs));
}

module.exports = { prepare, glorotInit, epochOrders, split, stack, saveModelFiles, DEFAULT_OPTIONS, prepareOrdinal, stackRegression, DEFAULT_OPTIONS_ORDS, WIDTHS, select, selectOrdinal };
