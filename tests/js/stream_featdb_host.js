// stream_featdb_host.js — drives js/formantanalyzer.js StreamOpen(..., {collect: db, names}) for tests/test_js_host_stream_featdb.py (spec FD-2).
// usage: node stream_featdb_host.js job.json -> JSON on stdout
//   job = {clips: [paths of raw float32 files, one per stream], fs, levels: [..], capacity, framesPerStep}
// Every stream is fed its clip step by step; stream 1 starts late, stream 2 is stopped and started again in the middle under a new name.  The
// callbacks go into the collector of js/featuredb.js under the name of the stream's launch; the device DB must export the same FeatureDB.
'use strict';
const fs = require('fs');
const path = require('path');
const JS = path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js');
const fa = require(path.join(JS, 'formantanalyzer.js'));
const { FeatureDB } = require(path.join(JS, 'featuredb.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const clips = job.clips.map((p) => { const b = fs.readFileSync(p); return new Float32Array(b.buffer, b.byteOffset, b.length / 4); });
const n = clips.length;
const message = (e) => (typeof e === 'string' ? e : String(e.message || e));

function one_level(level) {
  fa.configure(Object.assign({}, fa._settings, { output_level: level, devices: null }));
  const out = { level };
  const db = fa.createDeviceDB(level, job.capacity);
  const names = clips.map((_, i) => 'mic' + i);
  const host = new FeatureDB(), collect = host.collector(level, 1);
  let calls = 0;
  const h = fa.StreamOpen(n, job.fs, (si, label, t, f, s) => { calls++; collect(si, [names[s]], t, f); }, [], job.framesPerStep, 1024, null, { collect: db, names });
  const sps = h.samplesPerStep, steps = Math.floor(clips[0].length / sps), mid = Math.floor(steps / 2);
  let full = 0, grew = 0, before = 0;
  for (let k = 0; k < steps; k++) {
    const ctl = new Uint8Array(n);
    for (let i = 0; i < n; i++) {
      ctl[i] = i === 1 && k < 5 ? 0 : fa.STREAM_ACTIVE;
      if (k === (i === 1 ? 5 : 0)) ctl[i] |= fa.STREAM_START;
      if (k === steps - 1) ctl[i] |= fa.STREAM_STOP;
      h.input.set(clips[i].subarray(k * sps, (k + 1) * sps), i * sps);
    }
    if (k === mid) ctl[2] |= fa.STREAM_STOP;
    if (k === mid + 1) { ctl[2] |= fa.STREAM_START; h.rename(2, 'mic2 again'); names[2] = 'mic2 again'; }
    const r = h.push(ctl);
    if (r.dbFull) full++;
    if (db.records.length > before) grew++;
    before = db.records.length;
  }
  try { h.rename(0, 'mic1'); out.rename_again = null; } catch (e) { out.rename_again = message(e); }
  h.close();
  out.callbacks = calls; out.full = full; out.grew = grew;
  out.rows = db.count(); out.records = db.records.length;
  out.files = Array.from(new Set(db.records.map((r) => r.file)));
  const a = host.to_json(1), b = db.toFeatureDB(1).to_json(1);
  out.json_bytes = a === null ? 0 : a.length;
  out.json_equal = a === b;
  // the same names again: refused before a stream set exists
  try { fa.StreamOpen(n, job.fs, null, [], job.framesPerStep, 1024, null, { collect: db, names: ['x', 'mic0', 'y'] }); out.again = null; } catch (e) { out.again = message(e); }
  // setCollectDB's DB collects the sets opened without the argument; another level is refused
  if (level === 13) {
    const db2 = fa.createDeviceDB(13, job.capacity);
    fa.setCollectDB(db2);
    const h2 = fa.StreamOpen(n, job.fs, null, names.map((f) => [f + ' b']), job.framesPerStep);
    for (let k = 0; k < steps; k++) { for (let i = 0; i < n; i++) h2.input.set(clips[i].subarray(k * sps, (k + 1) * sps), i * sps); h2.push(); }
    h2.close();
    out.default_rows = db2.count(); out.default_records = db2.records.length;
    out.default_files = Array.from(new Set(db2.records.map((r) => r.file)));
    fa.setCollectDB(null);
    db2.close();
    const db5 = fa.createDeviceDB(5, 16);
    try { fa.StreamOpen(n, job.fs, null, [], job.framesPerStep, 1024, null, { collect: db5, names }); out.level_refusal = null; } catch (e) { out.level_refusal = message(e); }
    db5.close();
  }
  db.close();
  return out;
}

const results = [];
for (const level of job.levels) results.push(one_level(level));
fa.shutdown();
process.stdout.write(JSON.stringify(results));
