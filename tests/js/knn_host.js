// knn_host.js — drives js/formantanalyzer.js KNNClassifier / trainKnn / predictKnn for tests/test_js_host_knn.py.
// usage: node knn_host.js job.json -> JSON on stdout
//   job = {settings, case: {store, labels, queries, ks, split}, eval: [{key, rows: featuredb rows, label, classes, k}], clips: [f32 files], fs}
'use strict';
const fs = require('fs');
const path = require('path');
const js = path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js');
const fa = require(path.join(js, 'formantanalyzer.js'));
const { FeatureDB } = require(path.join(js, 'featuredb.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));

async function main() {
  fa.configure(Object.assign({}, fa._settings, job.settings));
  const out = { results: {}, evals: {}, refusals: {} };
  // one fixture case through ml5's own interface: the first `split` rows one addExample at a time, the rest at once
  const c = job.case, knn = fa.KNNClassifier(c.store[0].length, c.store.length);
  try { knn.classify(c.queries[0], 3); } catch (e) { out.refusals.empty = String(e); }
  for (let i = 0; i < c.split; i++) knn.addExample(c.store[i], c.labels[i]);
  out.classes_at_split = knn.names.slice();
  knn.addExamples(c.store.slice(c.split), c.labels.slice(c.split));
  out.classes = knn.names.slice(); out.counts = knn.getCountByLabel();
  for (const k of c.ks) {
    const r = fa.predictKnn(knn, c.queries, k), t = r.tables;
    out.results[k] = r.map((e, q) => ({ label: e.label, classIndex: e.classIndex, conf: knn.names.map((n) => e.confidencesByLabel[n]), byId: e.confidences,
                                        nbr: Array.from(t.nbr.subarray(q * t.k, q * t.k + t.kEff)) }));
  }
  out.one = knn.classify(c.queries[0], c.ks[0]);
  // the rows of a processed batch through batchKnn equal knnClassify over the rows the batch handed out
  if (job.clips) {
    const clips = job.clips.map((f) => ({ pcm: new Float32Array(fs.readFileSync(f).buffer.slice(0)), sampleRate: job.fs }));
    const rows = [];
    await fa.LaunchBatch(clips, (si, labels, time, feat) => { rows.push(Array.from(feat)); }, clips.map((_, i) => ['c' + i]));
    const viaBatch = knn.device.batch(knn.store, 3), direct = knn.device.classify(knn.store, Float64Array.from([].concat(...rows)), 3);
    out.batch = { rows: rows.length, same: ['label', 'conf', 'nbr', 'sim'].every((t) => Buffer.from(viaBatch[t].buffer).equals(Buffer.from(direct[t].buffer))) };
  }
  knn.release();
  try { knn.classify(c.queries[0], 3); } catch (e) { out.refusals.released = String(e); }
  for (const e of job.eval) {
    const db = new FeatureDB();
    db.from_json(1, JSON.stringify(e.rows));
    try {
      const r = fa.trainKnn(db, { db: 1, label: e.label, classes: e.classes, k: e.k });
      out.evals[e.key] = { samples: r.samples, correct: r.correct, all: r.all };
      r.knn.release();
    } catch (err) { out.evals[e.key] = { refused: String(err) }; }
  }
  process.stdout.write(JSON.stringify(out));
  if (fa.shutdown) fa.shutdown();
}
main().catch((e) => { console.error(e); process.exit(1); });
