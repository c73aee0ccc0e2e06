// napi_shapes_probe.js — the shape of every result object the addon hands to JavaScript, for tests/test_gpu_napi_shapes.py and
// tests/golden/gen/make_napi_shapes.py.
// usage: node napi_shapes_probe.js job.json  -> JSON on stdout
//   job = {addon, pcm: f32 file [n][ns], n, ns, fs, classifiers: [two cats_* directories], regress: [ords_* directories], frames_per_step}
//   out = {name: shape}: per result object its keys; per key [typed-array constructor, length], the number itself, or for `ens` the same one level down
'use strict';
const fs = require('fs');
const path = require('path');
const fa = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'formantanalyzer.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const nat = require(path.resolve(job.addon));
const ACTIVE = 1, START = 2, STOP = 4;

function shape(v) {
  if (ArrayBuffer.isView(v)) return [v.constructor.name, v.length];
  if (Array.isArray(v)) return v.map(shape);
  if (v !== null && typeof v === 'object') { const o = {}; for (const k of Object.keys(v).sort()) o[k] = shape(v[k]); return o; }
  return v === undefined ? 'undefined' : v;
}

async function main() {
  const out = {};
  const all = new Float32Array(fs.readFileSync(job.pcm).buffer.slice(0));
  const clips = [];
  for (let i = 0; i < job.n; i++) clips.push(all.slice(i * job.ns, (i + 1) * job.ns));
  const context = (level) => { const d = nat.defaults(); d.output_level = level; return nat.create(d, 0); };
  for (const level of [3, 4, 11]) {
    const c = context(level);
    out['batch_level_' + level] = shape(await nat.processBatch(c, clips, job.fs, level));
    nat.destroy(c);
  }
  const c = context(13);
  const cls = job.classifiers.map((d) => nat.modelCreate(c, fa.loadModel(d).spec));
  const reg_specs = job.regress.map((d) => fa.loadModel(d).spec);
  const reg = reg_specs.map((s) => nat.modelCreate(c, s));
  const lo = Float64Array.from(reg_specs, (s) => s.outMin), hi = Float64Array.from(reg_specs, (s) => s.outMax);
  const knn = nat.knnCreate(c, 53, 4, 8);
  out.knn_add = shape(nat.knnAdd(knn, Float64Array.from({ length: 6 * 53 }, (_, i) => 1 + (i % 7)), Int32Array.from([0, 1, 2, 3, 0, 1])));
  out.batch_level_13_model = shape(await nat.processBatch(c, clips, job.fs, 13, undefined, undefined, false, cls[0]));
  out.batch_level_13_ensemble = shape(await nat.processBatch(c, clips, job.fs, 13, undefined, undefined, false, cls));
  out.batch_level_13_plain = shape(await nat.processBatch(c, clips, job.fs, 13));
  out.batch_regress_group = shape(nat.batchRegressGroup(c, reg, lo, hi));
  out.batch_knn = shape(nat.batchKnn(c, knn, 3));
  out.batch_knn_fold = shape(nat.batchKnnFold(c));
  const attach = {
    model: (st) => nat.streamSetModel(st, cls[0]),
    knn: (st) => nat.streamSetKnn(st, knn, 3),
    ensemble: (st) => nat.streamSetEnsemble(st, cls),
    regress: (st) => nat.streamSetRegress(st, reg, lo, hi),
  };
  for (const what of Object.keys(attach)) {
    const st = nat.streamOpen(c, job.n, job.fs, job.frames_per_step, 1024);
    attach[what](st);
    const info = nat.streamInfo(st), sps = info.samplesPerStep, input = nat.streamInput(st), steps = Math.floor(job.ns / sps);
    const ctl = new Uint8Array(job.n);
    let first = null, last = null;
    for (let k = 0; k < steps; k++) {
      for (let i = 0; i < job.n; i++) input.set(clips[i].subarray(k * sps, (k + 1) * sps), i * info.inputStride);
      ctl.fill(ACTIVE | (k === 0 ? START : 0) | (k === steps - 1 ? STOP : 0));
      last = nat.streamStep(st, ctl);
      if (!first && last.meta.length) first = last;
    }
    out['stream_' + what + '_first_rows'] = shape(first);
    out['stream_' + what + '_last'] = shape(last);
    nat.streamClose(st);
  }
  nat.knnDestroy(knn);
  nat.destroy(c);
  fa.shutdown();
  process.stdout.write(JSON.stringify(out));
}
main().catch((e) => { console.error(e); process.exit(1); });
