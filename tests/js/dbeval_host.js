// dbeval_host.js — drives js/formantanalyzer.js evaluateDB over a FeatureDB for tests/test_js_host_dbeval.py.
// usage: node dbeval_host.js job.json -> JSON on stdout (NaN and the infinities as strings: JSON has none)
//   job = {rows, class_labels, ordinal_labels, models: {head: modelDir}, settings}
'use strict';
const fs = require('fs');
const path = require('path');
const js = path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js');
const fa = require(path.join(js, 'formantanalyzer.js'));
const { FeatureDB } = require(path.join(js, 'featuredb.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const enc = (k, v) => (typeof v === 'number' && !isFinite(v) ? String(v) : v);

function main() {
  fa.configure(Object.assign({}, fa._settings, job.settings));
  const db = new FeatureDB();
  db.from_json(1, JSON.stringify(job.rows));
  const heads = { db: 1, classLabels: job.class_labels, ordinalLabels: job.ordinal_labels }, out = { refusals: {} };
  out.result = fa.evaluateDB(db, Object.assign({ models: job.models }, heads));
  out.stored = JSON.parse(db.to_json(1)).map((r) => r.pred);
  out.rows_only = fa.evaluateDB(db, Object.assign({ perFile: false }, heads));          // no model: the predictions the samples now hold
  try { fa.evaluateDB(db, Object.assign({ models: { mood: job.models.emotion } }, heads)); } catch (e) { out.refusals.head = String(e); }
  try { fa.evaluateDB(db, Object.assign({ models: { emotion: job.models.V } }, heads)); } catch (e) { out.refusals.kind = String(e); }
  try { fa.evaluateDB(new FeatureDB(), heads); } catch (e) { out.refusals.empty = String(e); }
  process.stdout.write(JSON.stringify(out, enc));
  if (fa.shutdown) fa.shutdown();
}
try { main(); } catch (e) { console.error(e); process.exit(1); }
