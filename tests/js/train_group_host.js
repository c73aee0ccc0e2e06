// train_group_host.js — drives js/formantanalyzer.js trainModels against trainModel / trainRegression for tests/test_js_host_train_group.py.
// usage: node train_group_host.js job.json -> JSON on stdout
//   job = {classifier: {features, labels, classes, options, epochs, batchSize, seed}, regressor: {features, values, options, epochs, batchSize, seed},
//          extra: copies of the regressor's job to add (35 jobs in all: two consecutive groups), dir, settings}
'use strict';
const fs = require('fs');
const path = require('path');
const fa = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'formantanalyzer.js'));

const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const files = ['model.json', 'model_meta.json', 'model.weights.bin'];

async function main() {
  fa.configure(Object.assign({}, fa._settings, job.settings));
  const seen = { grouped: [[], []], single: [[], []] };
  const on = (list) => (e, st) => list.push([e, st.loss, st.acc, st.val_loss, st.val_acc]);
  const grouped = await fa.trainModels([
    Object.assign({}, job.classifier, { onEpoch: on(seen.grouped[0]) }),
    Object.assign({ regression: true }, job.regressor, { onEpoch: on(seen.grouped[1]) })]);
  const single = [
    await fa.trainModel(Object.assign({}, job.classifier, { onEpoch: on(seen.single[0]) })),
    await fa.trainRegression(job.regressor.features, job.regressor.values, Object.assign({}, job.regressor, { onEpoch: on(seen.single[1]) }))];
  const out = { seen, same_files: [], histories_equal: [], labels: grouped.map((h) => h.labels) };
  grouped.forEach((h, i) => {
    const a = path.join(job.dir, 'grouped', String(i)), b = path.join(job.dir, 'single', String(i));
    fa.saveModel(h, a); fa.saveModel(single[i], b);
    out.same_files.push(files.every((f) => fs.readFileSync(path.join(a, f)).equals(fs.readFileSync(path.join(b, f)))));
    out.histories_equal.push(JSON.stringify(h.history) === JSON.stringify(single[i].history) && h.history.length === [job.classifier, job.regressor][i].epochs);
  });
  // more than 32 jobs: consecutive groups, every handle still its own job's
  const many = [];
  for (let k = 0; k < job.extra; k++) many.push(Object.assign({ regression: true }, job.regressor, { epochs: 1 + (k % 2) }));
  const hs = await fa.trainModels(many);
  const one = await fa.trainRegression(job.regressor.features, job.regressor.values, Object.assign({}, job.regressor, { epochs: 1 }));
  const bytes = (h) => Buffer.concat(h.spec.kernels.concat(h.spec.biases).map((k) => Buffer.from(k.buffer, k.byteOffset, k.byteLength)));
  out.many = hs.length;
  out.many_epochs = hs.map((h) => h.history.length);
  out.many_equal = hs.every((h, k) => bytes(h).equals(bytes(k % 2 ? single[1] : one)));
  let refused = null;
  try { await fa.trainModels([job.classifier, Object.assign({}, job.classifier, { classes: job.classifier.classes.concat(['*']) })]); } catch (e) { refused = String(e); }
  out.wildcard = refused;
  process.stdout.write(JSON.stringify(out));
}
main().catch((e) => { console.error(e); process.exit(1); });
