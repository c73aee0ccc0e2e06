// classify_host.js — drives js/formantanalyzer.js with the app's classifier (loadModel / setPredictionModel / on_prediction) for
// tests/test_js_host_classify.py.  usage: node classify_host.js job.json  -> JSON on stdout
//   job = {mode: "excerpt", wav, settings, model}             one LaunchAudioNodes on a WAV file with the model set
//       | {mode: "stream", clips: [f32 file], fs, settings, model}  LaunchBatch without a model, with one, and after setPredictionModel(null)
//       | {mode: "release", model}                                 handles after shutdown() and after the context's destroy()
'use strict';
const fs = require('fs');
const path = require('path');
const fa = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'formantanalyzer.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = {};
const num = (x) => (Number.isFinite(x) ? x : String(x));

async function main() {
  if (job.mode === 'excerpt') {
    fa.configure(Object.assign({}, fa._settings, job.settings));
    const h = fa.loadModel(job.model);
    const preds = [], cbs = [];
    fa.setPredictionModel(h, (si, lc, clip, per) => preds.push({ si, pred: [lc[0], num(lc[1])], clip, per, after: cbs.length }));
    const r = await fa.LaunchAudioNodes(1, fs.readFileSync(job.wav), (si, label, t, f) => cbs.push(si), [], true, false);
    Object.assign(out, { resolved: r, callbacks: cbs, preds: preds.slice() });
    const b = await fa.LaunchBatch([fs.readFileSync(job.wav)], null, [], false);
    out.meters = b.meters;
  } else if (job.mode === 'stream') {
    fa.configure(Object.assign({}, fa._settings, job.settings));
    const clips = job.clips.map((f) => ({ pcm: new Float32Array(fs.readFileSync(f).buffer.slice(0)), sampleRate: job.fs }));
    const launch = async (tag) => {
      const cbs = [];
      const r = await fa.LaunchBatch(clips, (si, label, t, f, c) => cbs.push([si, label, t, f.map ? f.map((v) => (Array.isArray(v) ? v.map(num) : num(v))) : f, c]), clips.map((_, i) => ['c' + i]));
      out[tag] = { stream: JSON.stringify(cbs), resolved: JSON.stringify(Object.assign({}, r, { stageMs: null, meters: undefined })), meters: r.meters || null };
    };
    await launch('before');
    const h = fa.loadModel(job.model);
    const preds = [];
    fa.setPredictionModel(h, (si, lc, clip, per) => preds.push([si, lc[0], num(lc[1]), clip, Array.isArray(per[0]) ? per.length : 1]));
    await launch('with_model');
    out.preds = preds;
    fa.setPredictionModel(null);
    await launch('after');
  } else if (job.mode === 'release') {
    fa.configure(Object.assign({}, fa._settings, { output_level: 13 }));
    const h = fa.loadModel(job.model);
    fa.setPredictionModel(h, () => {});
    fa.setPredictionModel(null);
    fa.shutdown();
    try { fa.setPredictionModel(h, () => {}); out.after_shutdown = 'accepted'; } catch (e) { out.after_shutdown = String(e); }
    const nat = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'lib', 'wsa_napi.node'));
    const d = nat.defaults(); d.output_level = 13;
    const c = nat.create(d, 0);
    const m = nat.modelCreate(c, h.spec);
    nat.destroy(c);
    try { await nat.processBatch(c, [new Float32Array(16000)], 16000, 13, 16000, undefined, false, m); out.after_destroy = 'ran'; } catch (e) { out.after_destroy = String(e.message || e); }
    const c2 = nat.create(d, 0);
    try { await nat.processBatch(c2, [new Float32Array(16000)], 16000, 13, 16000, undefined, false, m); out.destroyed_model = 'ran'; } catch (e) { out.destroyed_model = String(e.message || e); }
    nat.modelDestroy(m); nat.modelDestroy(m);
    const m2 = nat.modelCreate(c2, h.spec);
    const c3 = nat.create(d, 0);
    try { await nat.processBatch(c3, [new Float32Array(16000)], 16000, 13, 16000, undefined, false, m2); out.other_ctx = 'ran'; } catch (e) { out.other_ctx = String(e.message || e); }
    nat.modelDestroy(m2); nat.destroy(c2); nat.destroy(c3);
  }
  process.stdout.write(JSON.stringify(out));
}
main().catch((e) => { console.error(e); process.exit(1); });
