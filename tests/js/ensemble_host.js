// ensemble_host.js — drives js/formantanalyzer.js with all of the app's model DBs (loadModel / setPredictionModels / on_prediction's detail)
// for tests/test_js_host_ensemble.py.  usage: node ensemble_host.js job.json  -> JSON on stdout
//   job = {wav, pcm48: f32 file (the same signal at fs48), fs48, settings, models: [dir, ...], silent: f32 file}
//   out = {batch: {preds, callbacks, meters, min_entropy_db, shown}, second: {...the same launch again}, silent: {npreds, meters, min_entropy_db, shown},
//          reversed: {preds, shown}, stream: {preds, meters, min_entropy_db}, single: {before, after}, refusals}
'use strict';
const fs = require('fs');
const path = require('path');
const fa = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'formantanalyzer.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = {};
const num = (x) => (Number.isFinite(x) ? x : String(x));
const meters_of = (m) => Object.keys(m).map((k) => [k, num(m[k])]);
const detail_of = (d) => ({ db: d.db, min_entropy_db: d.min_entropy_db, entropy: num(d.entropy), meters: meters_of(d.meters),
  per_db: d.per_db.map((p) => [p.label, num(p.confidence), Array.isArray(p.per_syllable[0]) ? p.per_syllable.length : 1]) });

async function batch(clip, handles) {
  const preds = [], cbs = [];
  fa.setPredictionModels(handles, (si, lc, c, d) => preds.push({ si, pred: [lc[0], num(lc[1])], clip: c, detail: detail_of(d), after: cbs.length }));
  const r = await fa.LaunchBatch([clip], (si) => cbs.push(si), [], false);
  return { preds, callbacks: cbs, meters: r.meters.map(meters_of), min_entropy_db: r.min_entropy_db, shown: r.shown_min_entropy_db };
}

async function main() {
  fa.configure(Object.assign({}, fa._settings, job.settings));
  const hs = job.models.map((m) => fa.loadModel(m));
  const wav = fs.readFileSync(job.wav);
  // setPredictionModel beside the new entry: the same launch before and after an ensemble was set
  const single = async () => {
    const p = [];
    fa.setPredictionModel(hs[0], (si, lc, c, per) => p.push([si, lc[0], num(lc[1]), c, Array.isArray(per[0]) ? per.length : 1]));
    const r = await fa.LaunchBatch([wav], null, [], false);
    return { preds: p, meters: r.meters, extra: [r.min_entropy_db === undefined, r.shown_min_entropy_db === undefined] };
  };
  out.single = { before: await single() };
  out.batch = await batch(wav, hs);
  out.second = await batch(wav, hs);
  // a launch without a callback: the device has no DB for it, the carried one stays
  const silent = { pcm: new Float32Array(fs.readFileSync(job.silent).buffer.slice(0)), sampleRate: job.fs48 };
  const s = await batch(silent, hs);
  out.silent = { npreds: s.preds.length, meters: s.meters, min_entropy_db: s.min_entropy_db, shown: s.shown };
  out.reversed = await batch(wav, [hs[1], hs[0]]);
  out.single.after = await single();
  // the same signal as one live source
  fa.configure(Object.assign({}, fa._settings, job.settings, { resample_to: 0 }));
  const pcm = new Float32Array(fs.readFileSync(job.pcm48).buffer.slice(0));
  const preds = [];
  fa.setPredictionModels(hs, (si, lc, c, d) => preds.push({ si, pred: [lc[0], num(lc[1])], clip: c, detail: detail_of(d) }));
  const h = fa.StreamOpen(1, job.fs48, null, [], 1);
  const sps = h.samplesPerStep, nsteps = Math.floor(pcm.length / sps);
  for (let k = 0; k < nsteps; k++) { h.input.set(pcm.subarray(k * sps, (k + 1) * sps)); h.push(); }
  const last = h.close();
  out.stream = { preds, meters: last.meters.map(meters_of), min_entropy_db: last.min_entropy_db };
  const b48 = await batch({ pcm: pcm.slice(0, nsteps * sps), sampleRate: job.fs48 }, hs);
  out.batch48 = b48;
  // refusals
  out.refusals = {};
  for (const [k, f] of Object.entries({ empty: () => fa.setPredictionModels([], () => {}), nine: () => fa.setPredictionModels(new Array(9).fill(hs[0]), () => {}),
    not_a_handle: () => fa.setPredictionModels([{}], () => {}), no_callback: () => fa.setPredictionModels(hs) })) {
    try { f(); out.refusals[k] = 'accepted'; } catch (e) { out.refusals[k] = String(e); }
  }
  fa.setPredictionModels(null);
  process.stdout.write(JSON.stringify(out));
}
main().catch((e) => { console.error(e); process.exit(1); });
