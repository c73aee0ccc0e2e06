// featdb_host.js — drives js/formantanalyzer.js createDeviceDB / setCollectDB / toFeatureDB / trainModel({db}) for tests/test_js_host_featdb.py.
// usage: node featdb_host.js job.json -> JSON on stdout
//   job = {clips: [paths of raw float32 files], fs, levels: [..], capacity, epochs, batchSize}
'use strict';
const fs = require('fs');
const path = require('path');
const JS = path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js');
const fa = require(path.join(JS, 'formantanalyzer.js'));
const { FeatureDB } = require(path.join(JS, 'featuredb.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const clips = job.clips.map((p) => { const b = fs.readFileSync(p); return { pcm: new Float32Array(b.buffer, b.byteOffset, b.length / 4), sampleRate: job.fs }; });
const files = job.clips.map((p) => path.basename(p));
const labels = files.map((f) => [f]);
const same_bytes = (a, b) => a.length === b.length && a.every((k, l) => Buffer.from(k.buffer, k.byteOffset, k.byteLength).equals(Buffer.from(b[l].buffer, b[l].byteOffset, b[l].byteLength)));
const message = (e) => (typeof e === 'string' ? e : String(e.message || e));

async function one_level(level) {
  fa.configure(Object.assign({}, fa._settings, { output_level: level, devices: null }));
  const out = { level };
  // the launch as it is today: callbacks into a FeatureDB through the collector
  const host = new FeatureDB(), collect = host.collector(level, 1), seen_a = [], vectors = [];
  await fa.LaunchBatch(clips, (si, label, t, f, ci) => {
    seen_a.push([si, label, t, f, ci]); collect(si, label, t, f);
    if (level === 13) f.forEach((v) => vectors.push(v));
  }, labels);
  // the same launch under setCollectDB: the same callbacks, and the DB filled on the device
  const db = fa.createDeviceDB(level, job.capacity);
  fa.setCollectDB(db);
  const seen_b = [];
  await fa.LaunchBatch(clips, (si, label, t, f, ci) => seen_b.push([si, label, t, f, ci]), labels);
  out.callbacks = seen_a.length;
  out.callbacks_equal = JSON.stringify(seen_a) === JSON.stringify(seen_b);
  out.rows = db.count();
  out.records = db.records.length;
  const a = host.to_json(1), b = db.toFeatureDB(1).to_json(1);
  out.json_bytes = a === null ? 0 : a.length;
  out.json_equal = a === b;
  // the same files again: refused before anything runs, the DB as it was
  try { await fa.LaunchBatch(clips, () => {}, labels); out.again = null; } catch (e) { out.again = message(e); }
  out.rows_after_refusal = db.count();
  if (level === 13) {
    // LaunchBatches while a DB collects: batch by batch on the DB's context, callbacks as ever
    const db2 = fa.createDeviceDB(level, job.capacity), host2 = new FeatureDB(), collect2 = host2.collector(level, 1);
    fa.setCollectDB(db2);
    const r = await fa.LaunchBatches(clips.map((c) => [c]), (si, label, t, f) => collect2(si, label, t, f), labels.map((l) => [l]));
    out.batches = r.batches;
    out.batches_json_equal = host2.to_json(1) === db2.toFeatureDB(1).to_json(1) && host2.to_json(1) === a;
    db2.close();
    fa.setCollectDB(null);
    // training from the device DB against training from the rows the callbacks delivered
    const lab = db.records.map((_, i) => (i % 5 === 4 ? null : ['low', 'high'][i % 2]));
    const common = { labels: lab, classes: ['low', 'high'], epochs: job.epochs, batchSize: job.batchSize, seed: 4 };
    const from_db = await fa.trainModel(Object.assign({ db }, common));
    const from_rows = await fa.trainModel(Object.assign({ features: vectors }, common));
    out.train_rows = vectors.length;
    out.train_equal = same_bytes(from_db.spec.kernels, from_rows.spec.kernels) && same_bytes(from_db.spec.biases, from_rows.spec.biases)
      && JSON.stringify(from_db.history) === JSON.stringify(from_rows.history) && JSON.stringify(from_db.labels) === JSON.stringify(from_rows.labels);
    out.train_loss = from_db.history.map((h) => h.loss);
    const values = db.records.map((_, i) => (i % 7 === 6 ? null : ((i * 13) % 17) / 16));
    const reg = { epochs: job.epochs, batchSize: job.batchSize, seed: 6 };
    const r_db = await fa.trainRegression(db, values, reg), r_rows = await fa.trainRegression(vectors, values, reg);
    out.regress_equal = same_bytes(r_db.spec.kernels, r_rows.spec.kernels) && same_bytes(r_db.spec.biases, r_rows.spec.biases) && r_db.spec.outMin === r_rows.spec.outMin;
    try { await fa.trainModel(Object.assign({ db }, common, { labels: lab.slice(1) })); out.short_labels = null; } catch (e) { out.short_labels = message(e); }
    // a device DB lives on one device, in one context
    fa.configure(Object.assign({}, fa._settings, { devices: [0, 1] }));
    try { fa.setCollectDB(db); out.multi = null; } catch (e) { out.multi = message(e); }
    // ... also where the list names one GPU twice (two contexts, two shards): setCollectDB refuses, and a launch refuses while a DB collects —
    // before anything runs, the DB and its files as they were
    fa.configure(Object.assign({}, fa._settings, { devices: [0, 0] }));
    try { fa.setCollectDB(db); out.twice = null; } catch (e) { out.twice = message(e); }
    fa.configure(Object.assign({}, fa._settings, { devices: null }));
    fa.setCollectDB(db);
    fa.configure(Object.assign({}, fa._settings, { devices: [0, 0] }));
    const more = clips.map((c) => ({ pcm: c.pcm.slice(), sampleRate: c.sampleRate })), more_labels = files.map((f) => ['again_' + f]);
    let calls = 0;
    try { await fa.LaunchBatch(more, () => { calls++; }, more_labels); out.twice_launch = null; } catch (e) { out.twice_launch = message(e); }
    out.twice_calls = calls;
    fa.configure(Object.assign({}, fa._settings, { devices: null }));
    out.rows_after_twice = db.count();
    out.records_after_twice = db.records.length;
    // the same new files on one context afterwards: taken (the refused launch marked none of them as held)
    await fa.LaunchBatch(more, () => {}, more_labels);
    out.rows_after_more = db.count();
    out.records_after_more = db.records.length;
  }
  fa.setCollectDB(null);
  db.close();
  return out;
}

async function main() {
  const out = [];
  for (const level of job.levels) out.push(await one_level(level));
  fa.shutdown();
  process.stdout.write(JSON.stringify(out));
}
main().catch((e) => { console.error(e); process.exit(1); });
