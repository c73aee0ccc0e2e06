// train_host.js — drives js/formantanalyzer.js trainModel / saveModel / setPredictionModel for tests/test_js_host_train.py.
// usage: node train_host.js job.json -> JSON on stdout
//   job = {features, labels, classes, options, epochs, batchSize, init: {kernels: [[..]], biases: [[..]]}, orders: [..], save_dir, wav, settings}
'use strict';
const fs = require('fs');
const path = require('path');
const fa = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'formantanalyzer.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

async function main() {
  fa.configure(Object.assign({}, fa._settings, job.settings));
  const epochs_seen = [];
  let ticks = 0;
  const timer = setInterval(() => { ticks++; }, 1);                 // the JS thread stays free while the epochs run
  const h = await fa.trainModel({ features: job.features, labels: job.labels, classes: job.classes, options: job.options, epochs: job.epochs,
    batchSize: job.batchSize, init: { kernels: job.init.kernels.map((k) => Float32Array.from(k)), biases: job.init.biases.map((b) => Float32Array.from(b)) },
    orders: Uint32Array.from(job.orders), onEpoch: (e, st) => epochs_seen.push([e, st.loss, st.acc, st.val_loss, st.val_acc]) });
  clearInterval(timer);
  const out = { kernels: h.spec.kernels.map((k) => Array.from(k)), biases: h.spec.biases.map((b) => Array.from(b)), labels: h.labels,
    history: h.history, epochs_seen, units: Array.from(h.spec.units) };
  fa.saveModel(h, job.save_dir);
  const preds = [];
  fa.setPredictionModel(h, (si, lc) => preds.push([si, lc[0], lc[1]]));
  out.resolved = await fa.LaunchAudioNodes(1, fs.readFileSync(job.wav), () => {}, [], true, false);
  out.preds = preds;
  // a seeded run without init / orders is repeatable
  const small = { features: job.features, labels: job.labels, classes: job.classes, options: job.options, epochs: 2, batchSize: job.batchSize, seed: 5 };
  const a = await fa.trainModel(small), b = await fa.trainModel(small);
  out.seeded_equal = a.spec.kernels.every((k, l) => Buffer.from(k.buffer).equals(Buffer.from(b.spec.kernels[l].buffer)));
  let refused = null;
  try { await fa.trainModel(Object.assign({}, small, { classes: job.classes.concat(['*']) })); } catch (e) { refused = String(e); }
  out.wildcard = refused;
  process.stdout.write(JSON.stringify(out));
}
main().catch((e) => { console.error(e); process.exit(1); });
