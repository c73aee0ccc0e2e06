// make_dbstats_golden.js — fixture generator helper for DB prediction and the results table (K8, specification DS-1).
// TEST INFRASTRUCTURE, build container only; tests/golden/gen/make_dbstats_golden.py writes the job and runs this script.
//
// Runs the reference application's OWN code, read AT RUN TIME (nothing of it is copied into this repository):
//   * /root/reference/src/localstore.js and src/labeling.js under the stub window.localStorage / document that
//     make_featuredb_golden.js uses: Load_JSON_Data, collect_db_data, update_pred_label, shows_stats_table;
//   * the text of nn_db_results_handler sliced out of src/neuralmodel.js (its storage_mod is the localstore object above);
//   * ml5 from dist/ml5.min.js (ml5 0.6.0 on tfjs 1.7.2, CPU backend): classify(row) / predict(row) per stored row, as
//     predict_db_nn calls them (src/neuralmodel.js:430-443).
// Per scenario it records ml5's per-row results, the `pred` pairs after the predictions and the results panel's text: one item
// per <li>, tags stripped, white space collapsed (the "Stats generated at" paragraph is no <li>).
// It ASSERTS the two conditions that make every comparison fair: every classified row's top-two margin exceeds 2e-5, and every
// printed minutes / RMSE text stays the same when its sum moves by +- 2 (n - 1) 2^-53 sum|terms| (and, for a head predicted by a
// regression model, when the RMSE moves by the tolerance K6's values are held to: "value_tol": {head: tol} of the scenario).
//
// usage: node make_dbstats_golden.js job.json out.json
//   job.json = {"ml5": ".../dist/ml5.min.js", "src": ".../src", "scenarios": [{"name", "class_labels", "ordinal_labels", "rows": [...],
//               "predict": [{"type": "cats"|"ords", "label", "dir", "task"}]}]}
'use strict';
const fs = require('fs');
const path = require('path');

const MARGIN = 2e-5;
const job = JSON.parse(fs.readFileSync(process.argv[2]));
const REF = job.src;

function strip_exports(src) { return src.replace(/^export\s+(async\s+)?function/gm, '$1function'); }

let store = new Map();
let dom = {};
const window_ = {
  localStorage: { getItem: k => (store.has(k) ? store.get(k) : null), setItem: (k, v) => { store.set(k, String(v)); },
                  removeItem: k => { store.delete(k); }, clear: () => store.clear() },
  URL: { createObjectURL: () => 'blob:x' }, navigator: {},
};
const document_ = {
  getElementById: id => { if (!dom[id]) dom[id] = { value: '', textContent: '', innerHTML: '', style: {} }; return dom[id]; },
  createElement: () => ({ click() {} }), body: { appendChild() {}, removeChild() {} },
};
const quiet = { log() {}, warn() {}, error() {} };

const lab = new Function('document', 'alert', 'console',
  strip_exports(fs.readFileSync(path.join(REF, 'labeling.js'), 'utf8')) + '\nreturn { Load_JSON_Labels_file, label_from_filename };')(document_, () => {}, quiet);
const ls = new Function('window', 'document', 'alert', 'Blob', 'require', 'setTimeout', 'console',
  strip_exports(fs.readFileSync(path.join(REF, 'localstore.js'), 'utf8')) + '\nreturn { collect_db_data, Load_JSON_Data, update_pred_label, shows_stats_table };')(
  window_, document_, () => {}, function () {}, () => lab, (f) => f(), quiet);
const nm = fs.readFileSync(path.join(REF, 'neuralmodel.js'), 'utf8');
const a = nm.indexOf('function nn_db_results_handler'), b = nm.indexOf('export function predict_single');
if (a < 0 || b < a) throw new Error('nn_db_results_handler not found');
const handler = new Function('storage_mod', 'label_types', 'document', 'console', 'var prediction_error = false;\n' + nm.slice(a, b) + '\nreturn nn_db_results_handler;')(
  ls, { cat: 'cats', ord: 'ords' }, document_, quiet);

function stub_dom() {
  const el = () => ({ getElementsByTagName: () => [], querySelector: () => null, querySelectorAll: () => [], removeChild() {},
                      getContext: () => null, style: {}, setAttribute() {}, appendChild() {}, insertBefore() {}, addEventListener() {},
                      sheet: { insertRule() {}, cssRules: [] }, childNodes: [], dataset: {}, innerHTML: '', textContent: '' });
  global.window = global; global.self = global;
  global.document = { createElement: el, createTextNode: el, getElementById: el, querySelector: () => null, addEventListener() {},
                      body: el(), head: el(), documentElement: el(), getElementsByTagName: () => [el()] };
  global.navigator = { userAgent: 'node', platform: 'node' };
}

async function load_model(ml5, dir, task) {
  const tf = ml5.tf;
  const mj = JSON.parse(fs.readFileSync(dir + '/model.json'));
  const meta = JSON.parse(fs.readFileSync(dir + '/model_meta.json'));
  const wb = fs.readFileSync(dir + '/model.weights.bin');
  const buf = wb.buffer.slice(wb.byteOffset, wb.byteOffset + wb.byteLength);
  const model = await tf.loadLayersModel(tf.io.fromMemory({ modelTopology: mj.modelTopology, weightSpecs: mj.weightsManifest[0].weights, weightData: buf }));
  const nn = ml5.neuralNetwork({ task, debug: false });
  nn.neuralNetwork.model = model; nn.neuralNetwork.isTrained = true;
  nn.neuralNetworkData.meta = meta; nn.neuralNetworkData.isMetadataReady = true;
  return nn;
}

const call = (nn, fn, row) => new Promise((res, rej) => nn[fn](row, (e, r) => (e ? rej(e) : res(r))));

function panel_items(html) {
  const items = [];
  for (const m of html.matchAll(/<li>([\s\S]*?)<\/li>/g)) items.push(m[1].replace(/<[^>]*>/g, ' ').replace(/\s+/g, ' ').trim());
  return items;
}

// the summation bound on every printed sum, on the rows as the reference's table sees them
function check_printed(data, heads_cat, heads_ord, value_tol) {
  const u = Math.pow(2, -53);
  for (const head of heads_cat) {
    const name = Object.keys(head)[0], sum = {}, abs = {}, cnt = {};
    for (let i = 0; i < data[0].length; i++) {
      const t = data[4][i];
      if (t && t[0][name] && (head[name].indexOf(t[0][name]) >= 0 || head[name].indexOf('*') >= 0)) {
        const k = t[0][name], d = parseFloat(data[1][i][1]);
        sum[k] = (sum[k] || 0) + d; abs[k] = (abs[k] || 0) + Math.abs(d); cnt[k] = (cnt[k] || 0) + 1;
      }
    }
    for (const k of Object.keys(sum)) {
      const bound = 2 * (cnt[k] - 1) * u * abs[k], text = (sum[k] / 60).toFixed(2);
      if (((sum[k] - bound) / 60).toFixed(2) !== text || ((sum[k] + bound) / 60).toFixed(2) !== text) throw new Error('minutes of ' + name + '/' + k + ' sit on a rounding edge');
    }
  }
  for (const name of heads_ord) {
    let s = 0, n = 0;
    for (let i = 0; i < data[0].length; i++) {
      const t = data[4][i], p = data[5][i];
      if (t && t[1][name] && !isNaN(t[1][name]) && p && p[1] && p[1][name] && !isNaN(p[1][name])) { s += Math.pow(p[1][name] - t[1][name], 2); n++; }
    }
    if (!n) continue;
    const bound = 2 * (n - 1) * u * s, text = Math.sqrt(s / n).toFixed(3);
    if (Math.sqrt((s - bound) / n).toFixed(3) !== text || Math.sqrt((s + bound) / n).toFixed(3) !== text) throw new Error('RMSE of ' + name + ' sits on a rounding edge');
    // predicted by a model: K6's values may differ from ml5's by value_tol per row, and the RMSE cannot move by more than that
    const tol = (value_tol || {})[name] || 0;
    if ((Math.sqrt(s / n) - tol).toFixed(3) !== text || (Math.sqrt(s / n) + tol).toFixed(3) !== text) throw new Error('RMSE of ' + name + ' is within the value tolerance of a rounding edge');
  }
}

async function main() {
  stub_dom();
  const ml5 = require(job.ml5);
  await ml5.tf.setBackend('cpu');
  const out = { generator: 'tests/golden/gen/make_dbstats_golden.js', node: process.version, ml5: ml5.version, tfjs: ml5.tf.version.tfjs,
                backend: ml5.tf.getBackend(), margin: MARGIN, scenarios: {} };
  for (const sc of job.scenarios) {
    store = new Map(); dom = {};
    document_.getElementById('class_labels').value = JSON.stringify(sc.class_labels);
    document_.getElementById('ordinal_labels').value = JSON.stringify(sc.ordinal_labels);
    const db = 1;
    ls.Load_JSON_Data(db, JSON.stringify(sc.rows));
    const recorded = [];
    for (const p of sc.predict) {
      const nn = await load_model(ml5, p.dir, p.task);
      const data = ls.collect_db_data(db);
      if (data[0].length !== sc.rows.length) throw new Error('rows lost on import');
      const results = [];
      for (let i = 0; i < data[0].length; i++) {
        const r = await call(nn, p.type === 'cats' ? 'classify' : 'predict', data[2][i]);
        handler(null, r, p.type, p.label, data[0][i]);
        if (p.type === 'cats') {
          const plain = r.map(e => ({ label: e.label, confidence: e.confidence }));
          if (plain.length > 1 && !(plain[0].confidence - plain[1].confidence > MARGIN)) throw new Error(sc.name + ' row ' + i + ': top-two margin ' + (plain[0].confidence - plain[1].confidence));
          results.push(plain);
        } else results.push(r[0].value);
      }
      recorded.push({ type: p.type, label: p.label, model: p.model, results });
    }
    const data = ls.collect_db_data(db);
    check_printed(data, sc.class_labels, sc.ordinal_labels, sc.value_tol);
    ls.shows_stats_table(null, db);
    out.scenarios[sc.name] = { class_labels: sc.class_labels, ordinal_labels: sc.ordinal_labels, rows: sc.rows, ml5: recorded,
                               pred_after: data[5], lines: panel_items(document_.getElementById('results_div').innerHTML) };
  }
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
}

main().catch(e => { console.error(e); process.exit(1); });
