// make_knn_golden.js — fixture generator helper for the KNN classifier (specification KN-1, kernel K9).  TEST INFRASTRUCTURE,
// build-container only.
//
// Loads the reference application's ml5 bundle (dist/ml5.min.js, ml5 0.6.0 on tfjs 1.7.2) AT RUN TIME — nothing of it is copied into
// this repository — and records what ml5.KNNClassifier() computes on the job's rows (tfjs CPU backend):
//   * per case: the class ids in the order of `for (key in classDatasetMatrices)`, the label ml5 reports for each, the grouped order
//     of the rows (which insertion index sits at which row of ml5's train matrix), every row's class, and ml5's own similarities
//     (knnClassifier.similarities) of every query, in that grouped order;
//   * per query and k: classify()'s label and confidences, and the neighbours tf.topk picks from those similarities — the call
//     predictClass itself makes — as insertion indices in selection order;
//   * per evaluation job: the (correct, all) figure of the app's train_knn procedure (ref src/neuralmodel.js:761-828), whose loop
//     over rows is restated here around ml5's addExample / classify (the function itself needs the app's storage module and DOM).
// make_knn_golden.py --exact sends the hand-built exact rows of tests/knn_exact_cases.py through run_case as they are, with each row's
// class index as a NUMBER label (ml5 takes a number as the class id itself), for tests/golden/knn_exact_expected.json.
// /root/reference does not exist on the GPU box: only tests/golden/gen/make_knn_golden.py runs this script.
//
// usage: node make_knn_golden.js job.json out.json
//   job.json = {"ml5": ".../dist/ml5.min.js",
//               "cases": [{"key": k, "store": [[...]], "labels": [...], "queries": [[...]], "ks": [...]}],
//               "evals": [{"key": k, "rows": [[...]], "labels": [label | null], "classes": [...], "k": 10}]}
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

// addExample, and which class id ml5 gave the row (read back from its per-class counts)
function add_tracked(knn, members, index, features, label) {
  const before = Object.assign({}, knn.knnClassifier.getClassExampleCount());
  knn.addExample(features, label);
  const after = knn.knnClassifier.getClassExampleCount();
  const grown = Object.keys(after).filter(key => after[key] !== (before[key] || 0));
  if (grown.length !== 1) throw new Error('addExample changed ' + grown.length + ' classes');
  (members[grown[0]] = members[grown[0]] || []).push(index);
}

async function run_case(ml5, c) {
  const tf = ml5.tf;
  const knn = ml5.KNNClassifier();
  const members = {};
  c.store.forEach((row, i) => add_tracked(knn, members, i, row, c.labels[i]));
  const keys = [];
  for (const key in knn.knnClassifier.classDatasetMatrices) keys.push(key);
  const grouped = [].concat(...keys.map(key => members[key]));
  const class_index = new Array(c.store.length);
  keys.forEach((key, ci) => members[key].forEach(i => { class_index[i] = ci; }));
  const names = keys.map(key => (knn.mapStringToIndex.length > 0 && knn.mapStringToIndex[key]) ? knn.mapStringToIndex[key] : key);
  const sims = [], results = [];
  for (const q of c.queries) {
    const sim = knn.knnClassifier.similarities(tf.tensor(q));
    sims.push(Array.from(sim.dataSync()));
    const per_k = {};
    for (const k of c.ks) {
      const r = await knn.classify(q, k);
      const k_eff = Math.min(k, grouped.length);
      const top = tf.topk(sim.asType('float32'), k_eff);
      per_k[k] = { label: String(r.label), class_index: r.classIndex, conf: keys.map(key => r.confidences[key]),
                   nbr: Array.from(top.indices.dataSync()).map(g => grouped[g]) };
    }
    results.push(per_k);
  }
  return { key: c.key, class_keys: keys, class_names: names, class_index, grouped, sims, results, counts: knn.getCountByLabel() };
}

// the app's procedure: the first parseInt(0.8 n) rows are added when they carry the label and it is listed (or '*' is), the next 100
// are classified with k; a row past the end has no label object and is skipped
async function run_eval(ml5, e) {
  const knn = ml5.KNNClassifier();
  const n = e.rows.length, split_at = parseInt(n * 0.8);
  const counts = i => i < n && e.labels[i] != null && (e.classes.indexOf(e.labels[i]) >= 0 || e.classes.indexOf('*') >= 0);
  let samples = 0;
  for (let i = 0; i < split_at; i++) if (counts(i)) { knn.addExample(e.rows[i], e.labels[i]); samples++; }
  if (samples < 10) return { key: e.key, refused: 'Sample size ' + String(samples) + '/' + String(n) + ' too small for training' };
  let all_n = 0, correct_n = 0;
  for (let i = split_at; i < split_at + 100; i++) {
    if (!counts(i)) continue;
    const r = await knn.classify(e.rows[i], e.k);
    all_n++;
    if (r.label == e.labels[i]) correct_n++;
  }
  return { key: e.key, samples, correct: correct_n, all: all_n };
}

async function main() {
  const job = JSON.parse(fs.readFileSync(process.argv[2]));
  stub_dom();
  const ml5 = require(job.ml5);
  await ml5.tf.setBackend('cpu');
  const out = { generator: 'tests/golden/gen/make_knn_golden.js', node: process.version, ml5: ml5.version, tfjs: ml5.tf.version.tfjs,
                backend: ml5.tf.getBackend(), cases: [], evals: [] };
  for (const c of job.cases) out.cases.push(await run_case(ml5, c));
  for (const e of job.evals) out.evals.push(await run_eval(ml5, e));
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
}

main().catch(e => { console.error(e); process.exit(1); });
