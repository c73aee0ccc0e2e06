// stream_values_host.js — drives js/formantanalyzer.js's StreamOpen and LaunchBatch with regression heads as value models (setPredictionValues) for
// tests/test_js_host_regress_live.py.
// usage: node stream_values_host.js job.json  -> JSON on stdout
//   job = {pcm: f32 file (one signal at fs), fs, settings, models: [ords_* directories], classifier: cats_* directory, frames_per_step,
//          hand: {meta, window_step, cb, value, cbValue, cbWeight, nHeads}: device tables of a hand-built case for the per-callback delivery alone}
//   out = {stream: {calls, values}, batch: {calls, values}, batches: {calls, values}, both: {order, calls_equal, preds}, hand: {calls}, refusals}
'use strict';
const fs = require('fs');
const path = require('path');
const fa = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'formantanalyzer.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = {};
const num = (x) => (Number.isFinite(x) ? x : String(x));
const nums = (a) => a.map(num);
const call_of = (si, v, unit, d) => [si, nums(v), unit, nums(d.weights), d.per_syllable.map(nums), nums(d.running)];
const values_of = (vs) => vs.map((u) => ({ sum: nums(u.sum), weight: nums(u.weight), value: nums(u.value) }));

function stream_run(pcm) {
  const calls = [];
  fa.setPredictionValues(handles, (si, v, s, d) => calls.push(call_of(si, v, s, d)));
  const h = fa.StreamOpen(1, job.fs, null, [], job.frames_per_step);
  const sps = h.samplesPerStep, nsteps = Math.floor(pcm.length / sps);
  for (let k = 0; k < nsteps; k++) {
    h.input.set(pcm.subarray(k * sps, (k + 1) * sps));
    h.push();
  }
  const last = h.close();
  return { calls, values: values_of(last.values), used: nsteps * sps };
}

let handles;
async function main() {
  fa.configure(Object.assign({}, fa._settings, job.settings));
  handles = job.models.map((d) => fa.loadModel(d));
  const cls = fa.loadModel(job.classifier);
  const raw = new Float32Array(fs.readFileSync(job.pcm).buffer.slice(0));
  const s = stream_run(raw);
  out.stream = { calls: s.calls, values: s.values };
  const pcm = raw.slice(0, s.used);
  const calls = [];
  fa.setPredictionValues(handles, (si, v, c, d) => calls.push(call_of(si, v, c, d)));
  const b = await fa.LaunchBatch([{ pcm, sampleRate: job.fs }], null, [], false);
  out.batch = { calls, values: values_of(b.values), meters: b.meters === undefined ? null : 'present' };
  // LaunchBatches: the same calls per batch (the batch index as the fifth argument) and values[batch][clip]
  const piped = [[], []];
  fa.setPredictionValues(handles, (si, v, c, d, k) => piped[k].push(call_of(si, v, c, d)));
  const bs = await fa.LaunchBatches([[{ pcm, sampleRate: job.fs }], [{ pcm, sampleRate: job.fs }]], null, [], false);
  out.batches = { calls: piped, values: bs.values.map(values_of) };
  // beside a prediction model: both handlers are called, the values after the prediction of the same callback, and the values do not change
  const order = [], again = [];
  fa.setPredictionModel(cls, (si) => order.push(['p', si]));
  fa.setPredictionValues(handles, (si, v, c, d) => { order.push(['v', si]); again.push(call_of(si, v, c, d)); });
  const b2 = await fa.LaunchBatch([{ pcm, sampleRate: job.fs }], (si) => order.push(['c', si]), [], false);
  out.both = { order, calls_equal: JSON.stringify(again) === JSON.stringify(calls), meters: Array.isArray(b2.meters), values: values_of(b2.values) };
  // setPredictionModel(null) leaves the value models alone, and the other way round
  fa.setPredictionModel(null);
  const kept = [];
  fa.setPredictionValues(handles, (si) => kept.push(si));
  await fa.LaunchBatch([{ pcm, sampleRate: job.fs }], null, [], false);
  fa.setPredictionValues(null);
  fa.setPredictionModel(cls, () => {});
  const b4 = await fa.LaunchBatch([{ pcm, sampleRate: job.fs }], null, [], false);
  out.independent = { values_kept: kept.length, after_null: b4.values === undefined && Array.isArray(b4.meters) };
  fa.setPredictionModel(null);
  // the per-callback delivery alone, over the device's tables of a hand-built case (skipped callbacks get no call)
  const H = job.hand, hand_calls = [], keep = fa._settings.window_step;
  fa._settings.window_step = H.window_step;
  try {
    const G = { cb: Int32Array.from(H.cb), value: Float64Array.from(H.value.map(Number)), cbValue: Float64Array.from(H.cbValue.map(Number)), cbWeight: Float64Array.from(H.cbWeight.map(Number)), nHeads: H.nHeads };
    const meta = Int32Array.from(H.meta), accs = new Map();
    const vp = { on_values: (si, v, u, d) => hand_calls.push(call_of(si, v, u, d)) };
    for (let k = 0; k < G.cb.length / 4; k++) fa._values_after(G, meta, G.cb[k * 4 + 2], G.cb[k * 4 + 1], G.cb[k * 4], vp, accs);
  } finally { fa._settings.window_step = keep; }
  out.hand = { calls: hand_calls };
  // refusals
  const refusals = {};
  const refused = (name, f) => { try { f(); refusals[name] = 'accepted'; } catch (e) { refusals[name] = String(e.message || e); } };
  refused('classifier', () => fa.setPredictionValues([cls], () => {}));
  refused('nine', () => fa.setPredictionValues(new Array(9).fill(handles[0]), () => {}));
  refused('none', () => fa.setPredictionValues([], () => {}));
  refused('no_handler', () => fa.setPredictionValues(handles));
  refused('regression_as_classifier', () => fa.setPredictionModel(handles[0], () => {}));
  fa.shutdown();
  refused('released', () => fa.setPredictionValues([handles[0]], () => {}));
  out.refusals = refusals;
  process.stdout.write(JSON.stringify(out));
}
main().catch((e) => { console.error(e); process.exit(1); });
