// knn.js — the host side of the app's ml5 KNN classifier (specification KN-1, K9): what src/neuralmodel.js:729-837 (train_knn) does around
// ml5.KNNClassifier() — which rows of a labelled feature DB are added, which are classified, the share that came out right — and ml5's
// own bookkeeping of labels (dist/ml5.min.js KNNClassifier.addExample / classifyInternal).  Everything that is a label is resolved here; the
// device sees class indices in ml5's class order.
//   * a STRING label gets the index of its first appearance (ml5's mapStringToIndex), a NUMBER label is its own class id;
//   * classes are scanned in the order of `for (key in classDatasetMatrices)`: ids that are array indices ascending, then any other in
//     order of first appearance.  With string labels alone that is the order of first appearance.
// device: {create(width, nClasses, capacity) -> store, add(store, Float64Array, Int32Array) -> {rows, perClass}, classify(store, Float64Array, k)
//          -> tables, destroy(store)} (formantanalyzer.js binds the addon's knnCreate / knnAdd / knnClassify / knnDestroy)
'use strict';

const MAX_CLASSES = 64, MAX_K = 64;        // WSA_MODEL_MAX_CLASSES, WSA_KNN_MAX_K
const WIDTHS = [53, 264, 23];

// {names, index}: the label ml5 reports for each class in scan order, and the class of every label
function labelOrder(labels) {
  const strings = [], seen = {}, per = [];
  for (const lab of labels) {
    let id;
    if (typeof lab === 'string') { id = strings.indexOf(lab); if (id < 0) id = strings.push(lab) - 1; }
    else if (typeof lab === 'number') id = lab;
    else throw 'KNN: a label is a string or a number, got ' + String(lab);
    seen[id] = true;                          // an object keeps its keys in the very order ml5's class table does
    per.push(String(id));
  }
  const keys = Object.keys(seen), pos = {};
  keys.forEach((k, i) => { pos[k] = i; });
  const names = keys.map((k) => (strings.length > 0 && strings[k] ? strings[k] : k));
  return { names, keys, index: Int32Array.from(per, (k) => pos[k]) };
}

// train_knn's choice of rows (ref neuralmodel.js:761-828): labels[i] is row i's value of the label (null / undefined: none)
function evaluationPlan(labels, classes) {
  const n = labels.length, splitAt = parseInt(n * 0.8);
  const counts = (i) => i < n && labels[i] != null && (classes.indexOf(labels[i]) >= 0 || classes.indexOf('*') >= 0);
  const add = [], test = [];
  for (let i = 0; i < splitAt; i++) if (counts(i)) add.push(i);
  if (add.length < 10) throw 'Sample size ' + String(add.length) + '/' + String(n) + ' too small for training';
  for (let i = splitAt; i < splitAt + 100; i++) if (counts(i)) test.push(i);
  return { add, test };
}

function pack(rows, width, who) {
  const x = new Float64Array(rows.length * width);
  rows.forEach((row, r) => {
    if (row.length !== width) throw who + ': row ' + r + ' has ' + row.length + ' features; ' + width + ' expected';
    for (let k = 0; k < width; k++) x[r * width + k] = Number(row[k]);
  });
  return x;
}

// ml5.KNNClassifier() on the device.  Keeps what was added: a label that sorts in front of stored classes (a number label below a stored
// one) renumbers them, and the store is then refilled.
class KnnClassifier {
  constructor(device, width, capacity) {
    if (WIDTHS.indexOf(width) < 0) throw 'KNN: rows of ' + width + ' features; 53 expected (or 264 at output_level 11, 23 at output_level 12)';
    this.device = device; this.width = width; this.capacity = capacity || 4096;
    this.store = device.create(width, MAX_CLASSES, this.capacity);
    this.rows = []; this.labels = []; this.index = new Int32Array(0); this.names = []; this.keys = [];
  }
  addExamples(rows, labels) {
    if (!this.store) throw 'KNN: the store was released';
    if (rows.length !== labels.length) throw 'KNN: ' + rows.length + ' rows, ' + labels.length + ' labels';
    const all = this.labels.concat(labels), o = labelOrder(all);
    if (o.names.length > MAX_CLASSES) throw 'KNN: ' + o.names.length + ' classes; a store takes ' + MAX_CLASSES;
    if (all.length > this.capacity) throw 'KNN: ' + all.length + ' rows; the store was created for ' + this.capacity;
    const old = this.labels.length;
    let same = true;
    for (let i = 0; i < old && same; i++) same = o.index[i] === this.index[i];
    this.rows = this.rows.concat(rows); this.labels = all;
    if (same) { if (rows.length) this.device.add(this.store, pack(rows, this.width, 'KNN'), o.index.slice(old)); }
    else {
      this.device.destroy(this.store);
      this.store = this.device.create(this.width, MAX_CLASSES, this.capacity);
      this.device.add(this.store, pack(this.rows, this.width, 'KNN'), o.index);
    }
    this.index = o.index; this.names = o.names; this.keys = o.keys;
  }
  addExample(features, label) { this.addExamples([features], [label]); }
  // ml5's results for `rows`: [{label, classIndex, confidences: {class id: c}, confidencesByLabel: {label: c}}] (+ the device's tables as `tables`)
  classifyMultiple(rows, k) {
    k = k === undefined ? 3 : k;            // ml5's default
    if (!this.store) throw 'KNN: the store was released';
    if (!this.labels.length) throw 'There is no example in any class';          // ml5's message
    const t = this.device.classify(this.store, pack(rows, this.width, 'KNN'), k), C = t.nClasses, nc = this.names.length;
    const out = rows.map((_, r) => {
      const ci = t.label[r], confidences = {}, byLabel = {};
      for (let c = 0; c < nc; c++) { confidences[this.keys[c]] = t.conf[r * C + c]; byLabel[this.names[c]] = t.conf[r * C + c]; }
      return { label: ci >= 0 ? this.names[ci] : null, classIndex: ci >= 0 ? Number(this.keys[ci]) : null, confidences, confidencesByLabel: byLabel };
    });
    out.tables = t;
    return out;
  }
  classify(features, k) { return this.classifyMultiple([features], k)[0]; }
  getCountByLabel() { const o = {}; this.names.forEach((n, c) => { o[n] = 0; }); this.index.forEach((c) => { o[this.names[c]]++; }); return o; }
  release() { if (this.store) { this.device.destroy(this.store); this.store = null; } }
}

// train_knn on a feature DB (featuredb.js): {knn, samples, correct, all} — the first 80 % of the DB's rows that carry `label` (and are listed in
// `classes`, or '*' is) are added, the next 100 are classified with k and compared as the app does (result.label == true_label)
function trainKnn(device, featureDB, o) {
  if (!o || !o.label || !Array.isArray(o.classes)) throw 'trainKnn(featureDB, {db, label, classes, k})';
  const samples = featureDB.samples(o.db);
  if (!samples.length) throw 'trainKnn: no data for training';
  const value = (s) => (s.truth && s.truth[0] && s.truth[0][o.label] != null ? s.truth[0][o.label] : null);
  const labels = samples.map(value), plan = evaluationPlan(labels, o.classes), k = o.k === undefined ? 10 : o.k;
  const knn = new KnnClassifier(device, samples[0].vector.length, plan.add.length);
  knn.addExamples(plan.add.map((i) => samples[i].vector), plan.add.map((i) => labels[i]));
  let correct = 0;
  if (plan.test.length) knn.classifyMultiple(plan.test.map((i) => samples[i].vector), k).forEach((r, j) => { if (r.label == labels[plan.test[j]]) correct++; });
  return { knn, samples: plan.add.length, correct, all: plan.test.length };
}

module.exports = { labelOrder, evaluationPlan, KnnClassifier, trainKnn, pack, MAX_K, MAX_CLASSES };
