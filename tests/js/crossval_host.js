// crossval_host.js — drives js/formantanalyzer.js crossValidate over a FeatureDB for tests/test_js_host_crossval.py.
// usage: node crossval_host.js job.json -> JSON on stdout (NaN and the infinities as strings: JSON has none)
//   job = {rows, class_labels, ordinal_labels, heads, k, epochs, batch_size, seed, inits, orders, models: {head: modelDir}, settings}
'use strict';
const fs = require('fs');
const path = require('path');
const js = path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js');
const fa = require(path.join(js, 'formantanalyzer.js'));
const { FeatureDB } = require(path.join(js, 'featuredb.js'));
const cv = require(path.join(js, 'crossval.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const enc = (k, v) => (typeof v === 'number' && !isFinite(v) ? String(v) : (ArrayBuffer.isView(v) ? Array.from(v) : v));

async function main() {
  fa.configure(Object.assign({}, fa._settings, job.settings));
  const load = () => { const db = new FeatureDB(); db.from_json(1, JSON.stringify(job.rows)); return db; };
  const heads = { db: 1, classLabels: job.class_labels, ordinalLabels: job.ordinal_labels }, out = { refusals: {} };
  // dbEval without foldOfRow: what evaluateDB gave before, on rows of their own
  const plainDb = load();
  out.plain = fa.evaluateDB(plainDb, Object.assign({ models: job.models }, heads));
  const db = load();
  const orders = {};
  for (const name of Object.keys(job.orders)) orders[name] = job.orders[name].map((o) => Uint32Array.from(o));
  const o = Object.assign({ heads: job.heads, k: job.k, epochs: job.epochs, batchSize: job.batch_size, seed: job.seed, inits: job.inits, orders, keepModels: true }, heads);
  const r = await fa.crossValidate(db, o);
  out.weights = {};
  for (const name of Object.keys(r.models)) out.weights[name] = r.models[name].map((h) => ({ kernels: h.spec.kernels.map((k) => Array.from(k)), biases: h.spec.biases.map((b) => Array.from(b)), labels: h.labels, history: h.history }));
  delete r.models;
  out.result = r;
  out.stored = JSON.parse(db.to_json(1)).map((row) => row.pred);
  out.folds = cv.assignFolds(db.samples(1), 2, (name) => name.split('_')[0]);
  try { await fa.crossValidate(db, Object.assign({}, o, { heads: ['mood'] })); } catch (e) { out.refusals.head = String(e); }
  try { await fa.crossValidate(db, Object.assign({}, o, { k: 33 })); } catch (e) { out.refusals.k = String(e); }
  try { await fa.crossValidate(db, Object.assign({}, o, { k: 9, groupOf: (name) => name.split('_')[0] })); } catch (e) { out.refusals.groups = String(e); }
  try { fa.evaluateDB(db, Object.assign({ models: { emotion: [] }, foldOfRow: r.foldOfRow, nFolds: 3 }, heads)); } catch (e) { out.refusals.members = String(e); }
  process.stdout.write(JSON.stringify(out, enc));
  if (fa.shutdown) fa.shutdown();
}
main().catch((e) => { console.error(e); process.exit(1); });
