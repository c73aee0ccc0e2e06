// make_regress_golden.js — fixture generator helper for regression training (K7 / specification TR-2).  TEST INFRASTRUCTURE,
// build-container only.
//
// Loads the reference application's ml5 bundle (dist/ml5.min.js, ml5 0.6.0 on tfjs 1.7.2) AT RUN TIME (nothing of it is copied
// into this repository), takes ml5.tf on the CPU backend and, per case, trains a tf.sequential of Dense layers compiled with exactly
// what ml5's `compile` passes for a regression task (meanSquaredError, tf.train.adam(learningRate), ["accuracy"]): the given initial
// weights, and per epoch one fit({batchSize, epochs: 1, shuffle: false, validationSplit}) over the training rows pre-ordered by that
// epoch's order with the validation rows left at the end.  The model and its optimizer live across the fits, as they do across the
// epochs of ml5's single fit: Adam's moments and accumulated betas carry over.  Records the history and every weight after every epoch.
//
// usage: node make_regress_golden.js job.json out.json
//   job.json = {"ml5": ".../dist/ml5.min.js", "cases": [{"key", "units", "activations", "kernels": [[[..]]], "biases": [[..]],
//               "x": [[53 normalised numbers]], "t": [normalised target], "n_val", "batch", "lr", "validation_split", "orders": [[..]]}]}
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
  if (!global.performance) global.performance = { now: () => Number(process.hrtime.bigint()) / 1e6 };   // fit's timers
  if (!global.requestAnimationFrame) global.requestAnimationFrame = f => setImmediate(() => f(Date.now()));
}

async function run_case(tf, c) {
  const nl = c.units.length - 1, n = c.x.length, n_train = n - c.n_val;
  const model = tf.sequential();
  for (let l = 0; l < nl; l++) {
    const cfg = { units: c.units[l + 1], activation: c.activations[l] };
    if (l === 0) cfg.inputShape = [c.units[0]];
    model.add(tf.layers.dense(cfg));
  }
  for (let l = 0; l < nl; l++)
    model.layers[l].setWeights([tf.tensor2d(c.kernels[l], [c.units[l], c.units[l + 1]], 'float32'), tf.tensor1d(c.biases[l], 'float32')]);
  model.compile({ loss: 'meanSquaredError', optimizer: tf.train.adam(c.lr), metrics: ['accuracy'] });
  const epochs = [];
  for (const order of c.orders) {
    const idx = order.concat(Array.from({ length: c.n_val }, (_, i) => n_train + i));
    const xs = tf.tensor2d(idx.map(i => c.x[i]), [n, c.units[0]], 'float32');
    const ys = tf.tensor2d(idx.map(i => [c.t[i]]), [n, 1], 'float32');
    const h = await model.fit(xs, ys, { batchSize: c.batch, epochs: 1, shuffle: false, validationSplit: c.validation_split, verbose: 0, yieldEvery: 'never' });
    xs.dispose(); ys.dispose();
    const rec = {};
    for (const k of Object.keys(h.history)) rec[k] = h.history[k][0];
    rec.kernels = []; rec.biases = [];
    for (let l = 0; l < nl; l++) {
      const w = model.layers[l].getWeights();
      rec.kernels.push(w[0].arraySync()); rec.biases.push(w[1].arraySync());
    }
    epochs.push(rec);
  }
  return { key: c.key, epochs, optimizer: model.optimizer.getClassName(), epsilon: model.optimizer.epsilon };
}

async function main() {
  const job = JSON.parse(fs.readFileSync(process.argv[2]));
  stub_dom();
  const ml5 = require(job.ml5);
  const tf = ml5.tf;
  await tf.setBackend('cpu');
  const out = { generator: 'tests/golden/gen/make_regress_golden.js', node: process.version, ml5: ml5.version, tfjs: tf.version.tfjs,
                backend: tf.getBackend(), cases: [] };
  for (const c of job.cases) out.cases.push(await run_case(tf, c));
  fs.writeFileSync(process.argv[3], JSON.stringify(out));
}

main().catch(e => { console.error(e); process.exit(1); });
