// make_fold_golden.js — fixture generator helper for the class fold alone (K6b / K6b-e on hand-built confidences).  TEST INFRASTRUCTURE,
// build-container only.
//
// Loads the reference application's src/prediction.js AT RUN TIME, as make_ensemble_golden.js does (nothing of it is copied into this
// repository), with `available_DBs` replaced by the case's list of members, and replaces nn_mod's classifier by a STUB that answers with the
// case's hand-built confidences in ml5 classifyMultiple's shape: per input the {label, confidence} entries in legend order, sorted with
// ml5's comparator (b.confidence - a.confidence) under this Node; with ONE input that input's list itself, not a one-element list
// (tests/test_classify_reference.py test_one_input_quirk_is_recorded).
//
// How that sort leaves equal and all-NaN confidences is not assumed: the generator first asks ml5's own classifyMultiple, through the
// throw-away model directories of job.probes (one Dense softmax layer with a zero kernel: equal biases give bit-equal probabilities, a NaN
// feature gives an all-NaN row), records the label order it answers with, and fails unless the stub gives the same order for the same
// confidences.
//
// The duration strings are Node's own ((t_len + 1) * step_s).toFixed(3).  Recorded per callback: callback_after_pred's [label, confidence]
// or null (no callback: the durations sum to 0), min_entropy_db, Label_conf_all of every member in Object.keys order, the gauges
// plot_prediction_meters draws (value = Label_conf_all[k] / all_class_sum, in key order) and its entropy text.  A NaN is written as the
// string "NaN" (JSON has none).
//
// usage: node make_fold_golden.js job.json out.json
//   job.json = {"ml5": ".../dist/ml5.min.js", "prediction": ".../src/prediction.js",
//               "probes": [{"name", "dir", "rows": [[..]]}],
//               "cases": [{"name", "step_s", "legends": [[..]], "callbacks": [{"t_len": [..], "conf": [member][syllable][class]}]}]}
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
const num = v => (v === 'NaN' ? NaN : v);
const enc = v => (typeof v === 'number' && v !== v ? 'NaN' : v);

// ml5's answer for hand-built confidences: entries in legend order, its comparator, its one-input shape
function stub_classify(legend, rows) {
  const g = rows.map(row => legend.map((label, c) => ({ [label]: row[c], label, confidence: row[c] })).sort(function (t, e) { return e.confidence - t.confidence; }));
  return g.length < 2 ? g[0] : g;
}

async function main() {
  const job = JSON.parse(fs.readFileSync(process.argv[2]));
  stub_dom();
  const ml5 = require(job.ml5);
  await ml5.tf.setBackend('cpu');
  const out = { generator: 'tests/golden/gen/make_fold_golden.js', node: process.version, ml5: ml5.version, tfjs: ml5.tf.version.tfjs,
                backend: ml5.tf.getBackend(), ml5_order: [], cases: [] };

  // 1. the order ml5 itself leaves equal and all-NaN confidences in; the stub must agree
  for (const p of job.probes) {
    const m = await load_model(ml5, p.dir);
    const rows = p.rows.map(r => r.map(num));
    for (const n of [rows.length, 1]) {             // several inputs, and the one-input shape
      let got = await classify(m.nn, rows.slice(0, n));
      const one_input_is_flat = n === 1 && !Array.isArray(got[0]);
      if (n === 1) got = [got];
      const conf = got.map(r => m.legend.map(l => r.find(e => e.label === l).confidence));
      let want = stub_classify(m.legend, conf);
      if (n === 1) want = [want];
      const order = got.map(r => r.map(e => e.label)), stub_order = want.map(r => r.map(e => e.label));
      if (JSON.stringify(order) !== JSON.stringify(stub_order)) throw new Error('the stub orders ' + p.name + ' as ' + JSON.stringify(stub_order) + ', ml5 as ' + JSON.stringify(order));
      out.ml5_order.push({ probe: p.name, inputs: n, one_input_is_flat, legend: m.legend, conf: conf.map(r => r.map(enc)), order });
    }
  }

  // 2. the cases through prediction.js with the stub
  for (const c of job.cases) {
    const dbs = c.legends.map((_, d) => d + 1);
    const nn_mod = { predict_single: (db_id, input, cb) => { cb(stub_classify(c.legends[db_id - 1], input.map(r => r[db_id - 1]))); } };
    const pred = load_prediction(job.prediction, nn_mod, dbs);
    pred.reset_predictions();
    const cbs = [];
    for (let k = 0; k < c.callbacks.length; k++) {
      const cb = c.callbacks[k];
      let t0 = 0;
      const seg_time = cb.t_len.map(t => { const d = ((t + 1) * c.step_s).toFixed(3); const st = [t0.toFixed(3), d]; t0 += parseFloat(d); return st; });
      // incoming: per syllable the members' confidence rows (what the stub reads; prediction.js only passes it on)
      const incoming = cb.t_len.map((_, ph) => c.legends.map((__, d) => cb.conf[d][ph].map(num)));
      plots.length = 0;
      const div = document.getElementById('speedometers_div');
      div.innerHTML = '';
      let got = null;
      pred.predict_by_multiple_syllables('cats', 'emotion', k, incoming, seg_time, (si, lc) => { got = lc; });
      await tick(); await tick(); await tick();     // the prediction's promises and plot_prediction_meters have run; no callback: seg_weight == 0
      const m = /Entropy: ([-0-9.A-Za-z]+)</.exec(div.innerHTML);
      const acc = pred.label_conf_all();
      cbs.push({ seg_time: seg_time.map(s => s[1]), pred: got ? got.map(enc) : null, min_entropy_db: pred.min_entropy_db(),
                 gauges: plots.map(p => [p.label, enc(p.value)]), entropy_text: m ? m[1] : null, entropy_red: /color:red/.test(div.innerHTML),
                 label_conf_all: dbs.map(db => Object.keys(acc[db]).map(key => [key, enc(acc[db][key])])) });
    }
    out.cases.push({ name: c.name, callbacks: cbs });
  }
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
}

main().catch(e => { console.error(e); process.exit(1); });
