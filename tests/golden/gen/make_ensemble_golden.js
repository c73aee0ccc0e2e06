// make_ensemble_golden.js — fixture generator helper for ensembles (K6e / K6b-e and the cross-DB decision).  TEST INFRASTRUCTURE,
// build-container only.
//
// Loads the reference application's ml5 bundle and its src/prediction.js AT RUN TIME, as make_classify_golden.js does (nothing of
// either is copied into this repository), with one more substitution: the line `const available_DBs = [1];` is replaced by the
// case's list of model DBs (the script fails if that line is not found).  predict_single dispatches on db_id to the loaded ml5
// models.  The DOM stub is persistent (getElementById returns one element per id) and plotly_lib.newPlot records its calls, so what
// plot_prediction_meters draws after every callback — the gauge values of min_entropy_db and the "Entropy: x.xxx" text — is stored
// next to callback_after_pred's [label, confidence] and min_entropy_db itself.  One prediction.js instance serves all clips of a
// case in order, reset_predictions() at each launch (src/index.js:395), so min_entropy_db carries over as it does in the app.
//
// usage: node make_ensemble_golden.js job.json out.json
//   job.json = {"ml5": ".../dist/ml5.min.js", "prediction": ".../src/prediction.js", "models": {"<db id>": "<dir>"},
//               "cases": [[1, 2], ...], "clips": [{"key": k, "callbacks": [{"si", "seg_time", "feat"}]}]}
'use strict';
const fs = require('fs');

const plots = [];
const elements = {};

function stub_dom() {
  const el = () => ({ getElementsByTagName: () => [], querySelector: () => null, querySelectorAll: () => [], removeChild() {},
                      getContext: () => null, style: {}, setAttribute() {}, appendChild() {}, insertBefore() {}, addEventListener() {},
                      sheet: { insertRule() {}, cssRules: [] }, childNodes: [], dataset: {}, innerHTML: '', textContent: '' });
  global.window = global; global.self = global;
  global.document = { createElement: el, createTextNode: el, getElementById: id => (elements[id] = elements[id] || el()), querySelector: () => null,
                      addEventListener() {}, body: el(), head: el(), documentElement: el(), getElementsByTagName: () => [el()] };
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

function load_prediction(path, nn_mod, dbs) {
  let src = fs.readFileSync(path, 'utf8');
  const lines = ["const nn_mod = require('./neuralmodel.js');", "const plotly_lib = require('plotly.js-finance-dist-min');", 'const available_DBs = [1];'];
  for (const s of lines) if (src.indexOf(s) < 0) throw new Error('prediction.js layout changed: ' + s);
  src = src.replace(lines[0], 'const nn_mod = __nn_mod;').replace(lines[1], 'const plotly_lib = __plotly;')
           .replace(lines[2], 'const available_DBs = ' + JSON.stringify(dbs) + ';');
  src = src.replace(/^export function/mg, 'function');
  src += '\nreturn { reset_predictions, predict_by_multiple_syllables, label_conf_all: () => Label_conf_all, min_entropy_db: () => min_entropy_db };\n';
  const plotly = { newPlot(id, data) { plots.push({ id, label: data[0].title.text, value: data[0].value }); } };
  return new Function('__nn_mod', '__plotly', src)(nn_mod, plotly);
}

const classify = (nn, rows) => new Promise((res, rej) => nn.classifyMultiple(rows, (e, r) => (e ? rej(e) : res(r))));
const tick = () => new Promise(res => setImmediate(res));

async function main() {
  const job = JSON.parse(fs.readFileSync(process.argv[2]));
  stub_dom();
  const ml5 = require(job.ml5);
  await ml5.tf.setBackend('cpu');
  const models = {};
  const out = { generator: 'tests/golden/gen/make_ensemble_golden.js', node: process.version, ml5: ml5.version, tfjs: ml5.tf.version.tfjs,
                backend: ml5.tf.getBackend(), legend: {}, prob: {}, cases: [] };
  const rows = [].concat(...job.clips.map(c => [].concat(...c.callbacks.map(cb => cb.feat))));
  for (const [db, dir] of Object.entries(job.models)) {
    const m = await load_model(ml5, dir);
    models[db] = m;
    out.legend[db] = m.legend;
    const all = await classify(m.nn, rows);
    out.prob[db] = all.map(r => m.legend.map(l => r.find(e => e.label === l).confidence));
  }
  const nn_mod = { predict_single: (db_id, input, cb) => { classify(models[db_id].nn, input).then(cb); } };
  for (const dbs of job.cases) {
    const pred = load_prediction(job.prediction, nn_mod, dbs);
    const clips = [];
    for (const c of job.clips) {
      pred.reset_predictions();
      const cbs = [];
      for (const cb of c.callbacks) {
        plots.length = 0;
        const div = document.getElementById('speedometers_div');
        div.innerHTML = '';
        const got = await new Promise(res => {
          let done = false;
          pred.predict_by_multiple_syllables('cats', 'emotion', cb.si, cb.feat, cb.seg_time, (si, lc) => { done = true; res({ si, pred: lc }); });
          setTimeout(() => { if (!done) res({ si: cb.si, pred: null }); }, 500);   // seg_weight == 0: no prediction, no callback
        });
        await tick(); await tick();               // plot_prediction_meters runs after callback_after_pred, in the same continuation
        const m = /Entropy: ([-0-9.A-Za-z]+)</.exec(div.innerHTML);
        cbs.push({ si: got.si, pred: got.pred, min_entropy_db: pred.min_entropy_db(), gauges: plots.map(p => [p.label, p.value]),
                   entropy_text: m ? m[1] : null, entropy_red: /color:red/.test(div.innerHTML) });
      }
      const acc = pred.label_conf_all();
      const conf = {};
      for (const db of dbs) conf[db] = Object.keys(acc[db]).map(k => [k, acc[db][k]]);
      clips.push({ key: c.key, callbacks: cbs, label_conf_all: conf });
    }
    out.cases.push({ dbs, clips });
  }
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
}

main().catch(e => { console.error(e); process.exit(1); });
