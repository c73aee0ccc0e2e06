// dbstats_host.js — drives js/formantanalyzer.js predictDB / statsTable over a FeatureDB for tests/test_js_host_dbstats.py.
// usage: node dbstats_host.js job.json -> JSON on stdout
//   job = {rows, class_labels, ordinal_labels, predict: [{type, label, modelDir}], settings}
'use strict';
const fs = require('fs');
const path = require('path');
const js = path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js');
const fa = require(path.join(js, 'formantanalyzer.js'));
const { FeatureDB } = require(path.join(js, 'featuredb.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

function main() {
  fa.configure(Object.assign({}, fa._settings, job.settings));
  const db = new FeatureDB();
  db.from_json(1, JSON.stringify(job.rows));
  const heads = { db: 1, classLabels: job.class_labels, ordinalLabels: job.ordinal_labels }, out = { preds: [], refusals: {} };
  for (const p of job.predict) out.preds.push(fa.predictDB(db, Object.assign({ type: p.type, label: p.label, modelDir: p.modelDir }, heads)));
  const table = fa.statsTable(db, heads);
  out.lines = table.lines; out.cats = table.cats; out.ords = table.ords;
  out.csv = db.to_csv(1); out.json = db.to_json(1);
  try { fa.predictDB(db, Object.assign({ type: 'ords', label: 'V', modelDir: job.predict[0].modelDir }, heads)); } catch (e) { out.refusals.kind = String(e); }
  try { fa.predictDB(new FeatureDB(), Object.assign({ type: 'cats', label: 'emotion', modelDir: job.predict[0].modelDir }, heads)); } catch (e) { out.refusals.empty = String(e); }
  process.stdout.write(JSON.stringify(out));
  if (fa.shutdown) fa.shutdown();
}
try { main(); } catch (e) { console.error(e); process.exit(1); }
