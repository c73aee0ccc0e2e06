// knn_refusals.js — setPredictionKnn's argument refusals (tests/test_knn_fold_host.py): none of them touches the addon, so a classifier over a
// stand-in device will do.  Prints the messages as JSON.
'use strict';
const path = require('path');
const fa = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'formantanalyzer.js'));
const K = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'knn.js'));
const device = { create: () => ({}), add: () => ({}), classify: () => { throw 'no device'; }, destroy: () => {} };
const row = Array.from({ length: 53 }, (_, i) => i + 1);
const filled = new K.KnnClassifier(device, 53, 4); filled.addExamples([row, row], ['a', 'b']);
const empty = new K.KnnClassifier(device, 53, 4);
const wide = new K.KnnClassifier(device, 264, 4);
const released = new K.KnnClassifier(device, 53, 4); released.addExamples([row], ['a']); released.release();
const cb = () => {};
const said = (f) => { try { f(); return null; } catch (e) { return String(e.message || e); } };
process.stdout.write(JSON.stringify({
  not_a_classifier: said(() => fa.setPredictionKnn({}, 10, cb)),
  wide: said(() => fa.setPredictionKnn(wide, 10, cb)),
  k0: said(() => fa.setPredictionKnn(filled, 0, cb)),
  k65: said(() => fa.setPredictionKnn(filled, 65, cb)),
  k_missing: said(() => fa.setPredictionKnn(filled, undefined, cb)),
  empty: said(() => fa.setPredictionKnn(empty, 10, cb)),
  released: said(() => fa.setPredictionKnn(released, 10, cb)),
  no_callback: said(() => fa.setPredictionKnn(filled, 10)),
  fine: said(() => fa.setPredictionKnn(filled, 10, cb)),
  detach: said(() => fa.setPredictionKnn(null)),
}));
