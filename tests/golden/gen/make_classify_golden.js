// make_classify_golden.js — fixture generator helper for the syllable classifier (K6 / K6b).  TEST INFRASTRUCTURE,
// build-container only.
//
// Loads the reference application's ml5 bundle (dist/ml5.min.js, ml5 0.6.0 on tfjs 1.7.2) and its src/prediction.js AT RUN
// TIME (nothing of either is copied into this repository), and records what they compute on the job's rows:
//   * per model, `classifyMultiple` over all rows in one call (tfjs CPU backend): the per-row probabilities in legend order,
//     and the sorted {label, confidence} lists as classifyMultiple returns them;
//   * per model and clip, prediction.js's own `predict_by_multiple_syllables` driven callback by callback (reset_predictions()
//     at each launch, as src/index.js:395 does; each callback's prediction awaited before the next one is handed in): the
//     [label, confidence] handed to callback_after_pred, the classifyMultiple result it folded, and the clip's Label_conf_all
//     accumulator in its key order.
// prediction.js is evaluated with its `export` keywords removed and its two imports replaced: neuralmodel.js by an object whose
// predict_single runs the loaded model's classifyMultiple (what src/neuralmodel.js:540 does once the model is loaded), plotly by
// a no-op.  /root/reference does not exist on the GPU box: only tests/golden/gen/make_classify_golden.py runs this script.
//
// usage: node make_classify_golden.js job.json out.json
//   job.json = {"ml5": ".../dist/ml5.min.js", "prediction": ".../src/prediction.js",
//               "models": {"<name>": "<dir holding model.json, model_meta.json, model.weights.bin>"},
//               "clips": [{"key": k, "callbacks": [{"si": si, "seg_time": [[start, dur], ...], "feat": [[53 numbers], ...]}]}]}
'use strict';
const fs = require('fs');

function stub_dom() {
  const el = () => ({ getElementsByTagName: () => [], querySelector: () => null, querySelectorAll: () => [], removeChild() {},
                      getContext: () => null, style: {}, setAttribute() {}, appendChild() {}, insertBefore() {}, addEventListener() {},
                      sheet: { insertRule() {}, cssRules: [] }, childNodes: [], dataset: {}, innerHTML: '', textContent: '' });
  global.window = global; global.self = global;
  global.document = { createElement: el, createTextNode: el, getElementById: el, querySelector: () => null, addEventListener() {},
                      body: el(), head: el(), documentElement: el(), getElementsByTagName: () => [el()] };
  global.navigator = { userAgent: 'node', platform: 'node' };
}

async function load_model(ml5, dir) {
  const tf = ml5.tf;
  const mj = JSON.parse(fs.readFileSync(dir + '/model.json'));
  const meta = JSON.parse(fs.readFileSync(dir + '/model_meta.json'));
  const wb = fs.readFileSync(dir + '/model.weights.bin');
  const buf = wb.buffer.slice(wb.byteOffset, wb.byteOffset + wb.byteLength);
  const model = await tf.loadLayersModel(tf.io.fromMemory({ modelTopology: mj.modelTopology, weightSpecs: mj.weightsManifest[0].weights, weightData: buf }));
  const nn = ml5.neuralNetwork({ task: 'classification', debug: false });
  nn.neuralNetwork.model = model; nn.neuralNetwork.isTrained = true;
  nn.neuralNetworkData.meta = meta; nn.neuralNetworkData.isMetadataReady = true;
  return { nn, legend: Object.keys(meta.outputs.y.legend) };
}

function load_prediction(path, state) {
  let src = fs.readFileSync(path, 'utf8');
  const imports = ["const nn_mod = require('./neuralmodel.js');", "const plotly_lib = require('plotly.js-finance-dist-min');"];
  for (const s of imports) if (src.indexOf(s) < 0) throw new Error('prediction.js layout changed: ' + s);
  src = src.replace(imports[0], 'const nn_mod = __nn_mod;').replace(imports[1], 'const plotly_lib = { newPlot() {} };');
  src = src.replace(/^export function/mg, 'function');
  src += '\nreturn { reset_predictions, predict_by_multiple_syllables, label_conf_all: () => Label_conf_all };\n';
  return new Function('__nn_mod', src)(state.nn_mod);
}

const classify = (nn, rows) => new Promise((res, rej) => nn.classifyMultiple(rows, (e, r) => (e ? rej(e) : res(r))));
const plain = r => (Array.isArray(r) ? r.map(plain) : { label: r.label, confidence: r.confidence });

async function main() {
  const job = JSON.parse(fs.readFileSync(process.argv[2]));
  stub_dom();
  const ml5 = require(job.ml5);
  await ml5.tf.setBackend('cpu');
  const state = { nn_mod: {}, current: null, last: null };
  state.nn_mod.predict_single = (db_id, input, cb) => {
    classify(state.current.nn, input).then(r => { state.last = plain(r); cb(r); });
  };
  const pred = load_prediction(job.prediction, state);
  const out = { generator: 'tests/golden/gen/make_classify_golden.js', node: process.version, ml5: ml5.version,
                tfjs: ml5.tf.version.tfjs, backend: ml5.tf.getBackend(), models: {} };
  for (const [name, dir] of Object.entries(job.models)) {
    const m = await load_model(ml5, dir);
    state.current = m;
    const rows = [].concat(...job.clips.map(c => [].concat(...c.callbacks.map(cb => cb.feat))));
    const all = await classify(m.nn, rows);
    const prob = all.map(r => m.legend.map(l => r.find(e => e.label === l).confidence));
    const one = plain(await classify(m.nn, [rows[0]]));   // the one-input quirk: the sorted array itself
    const clips = [];
    for (const c of job.clips) {
      pred.reset_predictions();
      const cbs = [];
      for (const cb of c.callbacks) {
        const got = await new Promise(res => {
          let done = false;
          state.last = null;
          pred.predict_by_multiple_syllables('cats', 'emotion', cb.si, cb.feat, cb.seg_time, (si, lc) => { done = true; res({ si, pred: lc }); });
          setTimeout(() => { if (!done) res({ si: cb.si, pred: null }); }, 200);   // seg_weight == 0: no prediction, no callback
        });
        cbs.push({ si: got.si, pred: got.pred, ml5: state.last });
      }
      const acc = pred.label_conf_all()[1];
      clips.push({ key: c.key, callbacks: cbs, clip_conf: Object.keys(acc).map(k => [k, acc[k]]) });
    }
    out.models[name] = { legend: m.legend, prob, one_input: one, clips };
  }
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
}

main().catch(e => { console.error(e); process.exit(1); });
