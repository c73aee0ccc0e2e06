// regress_host.js — drives js/formantanalyzer.js trainRegression / saveModel / loadModel / predictValues for tests/test_js_host_regress.py.
// usage: node regress_host.js job.json -> JSON on stdout
//   job = {features, values, options, epochs, batchSize, init: {kernels: [[..]], biases: [[..]]}, orders: [..], save_dir, rows, settings}
'use strict';
const fs = require('fs');
const path = require('path');
const fa = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'formantanalyzer.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

async function main() {
  fa.configure(Object.assign({}, fa._settings, job.settings));
  const epochs_seen = [];
  const h = await fa.trainRegression(job.features, job.values, { options: job.options, epochs: job.epochs, batchSize: job.batchSize,
    init: { kernels: job.init.kernels.map((k) => Float32Array.from(k)), biases: job.init.biases.map((b) => Float32Array.from(b)) },
    orders: Uint32Array.from(job.orders), onEpoch: (e, st) => epochs_seen.push([e, st.loss, st.acc, st.val_loss, st.val_acc]) });
  const out = { kernels: h.spec.kernels.map((k) => Array.from(k)), biases: h.spec.biases.map((b) => Array.from(b)), history: h.history, epochs_seen,
    units: Array.from(h.spec.units), outMin: h.spec.outMin, outMax: h.spec.outMax, labels: h.labels };
  fa.saveModel(h, job.save_dir);
  out.values = Array.from(fa.predictValues(h, job.rows));
  out.values_loaded = Array.from(fa.predictValues(fa.loadModel(job.save_dir), job.rows));
  const refusals = {};
  try { await fa.trainModel({ features: job.features, labels: job.values.map(String), classes: ['0.2', '0.8'], options: job.options, epochs: 1 }); } catch (e) { refusals.train_model = String(e); }
  try { await fa.trainRegression(job.features.slice(10, 19), job.values.slice(10, 19), {}); } catch (e) { refusals.nine_rows = String(e); }
  try { fa.setPredictionModel(h, () => {}); } catch (e) { refusals.set_prediction = String(e); }
  out.refusals = refusals;
  process.stdout.write(JSON.stringify(out));
}
main().catch((e) => { console.error(e); process.exit(1); });
