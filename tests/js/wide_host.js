// wide_host.js — drives js/formantanalyzer.js trainModel / saveModel / loadModel / predictDB on 264-wide rows (the utterance vectors of
// output_level 11, stored through featuredb.js as the app stores them) for tests/test_js_host_wide.py.
// usage: node wide_host.js job.json -> JSON on stdout
//   job = {features: [[264 numbers]], labels, classes, options, epochs, batchSize, init: {kernels, biases}, orders, save_dir, label}
'use strict';
const fs = require('fs');
const path = require('path');
const js = path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js');
const fa = require(path.join(js, 'formantanalyzer.js'));
const { FeatureDB } = require(path.join(js, 'featuredb.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

async function main() {
  fa.configure(Object.assign({}, fa._settings, { output_level: 11 }));
  const db = new FeatureDB();
  job.features.forEach((v, i) => { if (!db.put(11, 1, 'file' + i + '.wav', 0, [0, 0.5 + i / 100], v)) throw 'put refused: ' + db.refused.join('; '); });
  const h = await fa.trainModel({ features: job.features, labels: job.labels, classes: job.classes, options: job.options, epochs: job.epochs,
    batchSize: job.batchSize, init: { kernels: job.init.kernels.map((k) => Float32Array.from(k)), biases: job.init.biases.map((b) => Float32Array.from(b)) },
    orders: Uint32Array.from(job.orders) });
  const out = { units: Array.from(h.spec.units), kernels: h.spec.kernels.map((k) => Array.from(k)), biases: h.spec.biases.map((b) => Array.from(b)),
    labels: h.labels, history: h.history, refusals: {} };
  fa.saveModel(h, job.save_dir);
  const back = fa.loadModel(job.save_dir);
  out.loaded_units = Array.from(back.spec.units);
  out.loaded_equal = back.spec.kernels.every((k, l) => Buffer.from(k.buffer, k.byteOffset, k.byteLength).equals(Buffer.from(h.spec.kernels[l].buffer, h.spec.kernels[l].byteOffset, h.spec.kernels[l].byteLength)));
  out.preds = fa.predictDB(db, { db: 1, type: 'cats', label: job.label, model: back, classLabels: [{ [job.label]: job.classes }], ordinalLabels: [] });
  out.stored = db.samples(1).map((s) => s.guess);
  try { fa.setPredictionModel(back, () => {}); } catch (e) { out.refusals.set_model = String(e); }
  try { fa.setPredictionModels([back], () => {}); } catch (e) { out.refusals.set_models = String(e); }
  const narrow = new FeatureDB();
  narrow.put(5, 1, 'a.wav', 0, [0, 1], new Array(53).fill(0.5));
  try { fa.predictDB(narrow, { db: 1, type: 'cats', label: job.label, model: back, classLabels: [{ [job.label]: job.classes }], ordinalLabels: [] }); } catch (e) { out.refusals.width = String(e); }
  process.stdout.write(JSON.stringify(out));
  if (fa.shutdown) fa.shutdown();
}
main().catch((e) => { console.error(e); process.exit(1); });
