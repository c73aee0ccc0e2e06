// make_dbeval_golden.js — fixture generator helper for the evaluation of a labelled DB (specification EV-1, K8e).  TEST INFRASTRUCTURE,
// build-container only.
//
// Loads the reference application's src/stats.js and src/prediction.js AT RUN TIME (nothing of them is copied into this repository):
//   * stats.js for only_mean / variance / covariance, which it runs over each ordinal case's pairs — the pairs that pass DS-1's device
//     rule in both columns, selected here — and the CCC expression of calc_ccc (src/neuralmodel.js:488) with covariance(y1, y2), plus
//     Pearson's r from the same three;
//   * prediction.js as make_fold_golden.js loads it, with nn_mod's classifier replaced by a STUB that answers with the case's fixed
//     probability tables in ml5 classifyMultiple's shape (how ml5 orders equal confidences is pinned by make_fold_golden.js against ml5
//     itself; the stub is that one).  Every file of a case is one launch: reset_predictions(), then each callback through
//     predict_by_multiple_syllables; Label_conf_all after the file's last callback is recorded in Object.keys order.
// The duration strings are (ms / 1000).toFixed(3).  A NaN is written as the string "NaN", an infinity as "Infinity" / "-Infinity".
//
// usage: node make_dbeval_golden.js job.json out.json
//   job.json = {"stats": ".../src/stats.js", "prediction": ".../src/prediction.js",
//               "ordinal": [{"name", "true": [..], "pred": [..]}], "fold": [{"name", "legend", "files": [[{"dur_ms", "prob"}]]}]}
'use strict';
const fs = require('fs');

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

function load_stats(path) {
  let src = fs.readFileSync(path, 'utf8');
  for (const s of ['export const only_mean', 'export function covariance', 'export function variance']) if (src.indexOf(s) < 0) throw new Error('stats.js layout changed: ' + s);
  src = src.replace(/^export /mg, '');
  src += '\nreturn { only_mean, variance, covariance };\n';
  return new Function(src)();
}

function load_prediction(path, nn_mod) {
  let src = fs.readFileSync(path, 'utf8');
  const lines = ["const nn_mod = require('./neuralmodel.js');", "const plotly_lib = require('plotly.js-finance-dist-min');", 'const available_DBs = [1];'];
  for (const s of lines) if (src.indexOf(s) < 0) throw new Error('prediction.js layout changed: ' + s);
  src = src.replace(lines[0], 'const nn_mod = __nn_mod;').replace(lines[1], 'const plotly_lib = __plotly;');
  src = src.replace(/^export function/mg, 'function');
  src += '\nreturn { reset_predictions, predict_by_multiple_syllables, label_conf_all: () => Label_conf_all };\n';
  return new Function('__nn_mod', '__plotly', src)(nn_mod, { newPlot() {} });
}

const tick = () => new Promise(res => setImmediate(res));
const num = v => (v === 'NaN' ? NaN : v === 'Infinity' ? Infinity : v === '-Infinity' ? -Infinity : v);
const enc = v => (typeof v !== 'number' ? v : v !== v ? 'NaN' : v === Infinity ? 'Infinity' : v === -Infinity ? '-Infinity' : v);
const counted = v => v === v && v !== 0;     // DS-1's device rule: truthy and not NaN

// ml5's answer for fixed confidences: entries in legend order, its comparator, its one-input shape (make_fold_golden.js)
function stub_classify(legend, rows) {
  const g = rows.map(row => legend.map((label, c) => ({ [label]: row[c], label, confidence: row[c] })).sort(function (t, e) { return e.confidence - t.confidence; }));
  return g.length < 2 ? g[0] : g;
}

async function main() {
  const job = JSON.parse(fs.readFileSync(process.argv[2]));
  stub_dom();
  const stats = load_stats(job.stats);
  const out = { generator: 'tests/golden/gen/make_dbeval_golden.js', node: process.version, ordinal: [], fold: [] };

  for (const c of job.ordinal) {
    const y1 = [], y2 = [];
    c.true.forEach((t, i) => { const a = num(t), b = num(c.pred[i]); if (counted(a) && counted(b)) { y1.push(a); y2.push(b); } });
    const y1_mean = stats.only_mean(y1), y2_mean = stats.only_mean(y2), y1_var = stats.variance(y1), y2_var = stats.variance(y2);
    const co_var = stats.covariance(y1, y2);
    const ccc_val = (2 * co_var) / (y1_var + y2_var + Math.pow(y2_mean - y1_mean, 2));
    out.ordinal.push({ name: c.name, n: y1.length, mean_true: enc(y1_mean), mean_pred: enc(y2_mean), var_true: enc(y1_var), var_pred: enc(y2_var),
                       cov: enc(co_var), ccc: enc(ccc_val), pearson: enc(co_var / Math.sqrt(y1_var * y2_var)),
                       cov_y1_y1: enc(stats.covariance(y1, y1)) });       // what calc_ccc itself passes: the variance again
  }

  for (const c of job.fold) {
    const nn_mod = { predict_single: (db_id, input, cb) => { cb(stub_classify(c.legend, input.map(r => r[0]))); } };
    const pred = load_prediction(job.prediction, nn_mod);
    const files = [];
    for (const cbs of c.files) {
      pred.reset_predictions();
      const answers = [];
      for (let k = 0; k < cbs.length; k++) {
        const cb = cbs[k];
        let t0 = 0;
        const seg_time = cb.dur_ms.map(ms => { const d = (ms / 1000).toFixed(3); const st = [t0.toFixed(3), d]; t0 += parseFloat(d); return st; });
        const incoming = cb.prob.map(row => [row.map(num)]);
        let got = null;
        pred.predict_by_multiple_syllables('cats', 'emotion', k, incoming, seg_time, (si, lc) => { got = lc; });
        await tick(); await tick(); await tick();
        answers.push(got ? got.map(enc) : null);
      }
      const acc = pred.label_conf_all()[1] || {};
      files.push({ callbacks: answers, label_conf_all: Object.keys(acc).map(key => [key, enc(acc[key])]) });
    }
    out.fold.push({ name: c.name, files });
  }
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
}

main().catch(e => { console.error(e); process.exit(1); });
