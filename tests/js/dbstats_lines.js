// dbstats_lines.js — js/dbstats.js without a device, for tests/test_dbstats_host.py: the fixture's rows with the reference's `pred` pairs go through
// columns(), a plain in-order count of those columns stands in for the device's table, and assemble() / lines() print it.
// usage: node dbstats_lines.js tests/golden/dbstats_expected.json -> {scenario: [lines]} on stdout
'use strict';
const fs = require('fs');
const path = require('path');
const js = path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js');
const { FeatureDB } = require(path.join(js, 'featuredb.js'));
const ds = require(path.join(js, 'dbstats.js'));

function count(col) {
  const n = col.n, items = col.vocab.reduce((a, b) => a + b, 0), nOrd = col.ordNames.length;
  const cat = new Float64Array(col.vocab.length * 3), cls = new Float64Array(items * 5), ord = new Float64Array(nOrd * 5);
  for (let i = 0; i < items; i++) cls[i * 5 + 4] = 4294967295;
  let off = 0;
  col.vocab.forEach((V, h) => {
    for (let i = 0; i < n; i++) {
      const t = col.trueIdx[h * n + i], p = col.predIdx[h * n + i];
      if (t < 0) continue;
      const e = (off + t) * 5;
      if (cls[e] === 0) cls[e + 4] = i;
      cls[e]++; cls[e + 3] += col.durations[i];
      if (p < 0) cat[h * 3 + 2]++;
      else if (p === t) { cls[e + 1]++; cat[h * 3]++; } else { cls[e + 2]++; cat[h * 3 + 1]++; }
    }
    off += V;
  });
  for (let o = 0; o < nOrd; o++) {
    ord[o * 5 + 2] = Infinity;
    for (let i = 0; i < n; i++) {
      const t = col.trueVal[o * n + i], p = col.predVal[o * n + i];
      if (!(t === t && t !== 0)) continue;
      ord[o * 5]++;
      if (t < ord[o * 5 + 2]) ord[o * 5 + 2] = t;
      if (t > ord[o * 5 + 3]) ord[o * 5 + 3] = t;
      if (p === p && p !== 0) { ord[o * 5 + 1]++; ord[o * 5 + 4] += (p - t) * (p - t); }
    }
  }
  return { cat, cls, ord };
}

const fx = JSON.parse(fs.readFileSync(process.argv[2], 'utf8')), out = {};
for (const [name, sc] of Object.entries(fx.scenarios)) {
  const db = new FeatureDB();
  db.from_json(1, JSON.stringify(sc.rows));
  db.samples(1).forEach((s, i) => { s.guess = sc.pred_after[i]; });
  out[name] = ds.statsTable({ table: count }, db, { db: 1, classLabels: sc.class_labels, ordinalLabels: sc.ordinal_labels }).lines;
}
process.stdout.write(JSON.stringify(out));
