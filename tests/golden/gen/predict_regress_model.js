// predict_regress_model.js — loads a regression model directory (model.json, model_meta.json, model.weights.bin) into the REFERENCE
// application's own ml5 bundle under Node and runs predictMultiple over given rows.  TEST INFRASTRUCTURE, build-container only: the
// bundle (dist/ml5.min.js, ml5 0.6.0 on tfjs 1.7.2) is loaded AT RUN TIME, nothing of it is copied into this repository.
// What src/neuralmodel.js:540-585 (predict_single) does once an ords_<label> model is loaded: result[0].value per row.
//
// usage: node predict_regress_model.js job.json out.json
//   job.json = {"ml5": ".../dist/ml5.min.js", "dir": "<model directory>", "feat": [[53 numbers], ...]}
//   out.json = {"value": [..], "unnormalised_from": [..], "meta_outputs": {...}}
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

async function main() {
  const job = JSON.parse(fs.readFileSync(process.argv[2]));
  stub_dom();
  const ml5 = require(job.ml5);
  const tf = ml5.tf;
  await tf.setBackend('cpu');
  const mj = JSON.parse(fs.readFileSync(job.dir + '/model.json'));
  const meta = JSON.parse(fs.readFileSync(job.dir + '/model_meta.json'));
  const wb = fs.readFileSync(job.dir + '/model.weights.bin');
  const buf = wb.buffer.slice(wb.byteOffset, wb.byteOffset + wb.byteLength);
  const model = await tf.loadLayersModel(tf.io.fromMemory({ modelTopology: mj.modelTopology, weightSpecs: mj.weightsManifest[0].weights, weightData: buf }));
  const nn = ml5.neuralNetwork({ task: 'regression', debug: false });
  nn.neuralNetwork.model = model; nn.neuralNetwork.isTrained = true;
  nn.neuralNetworkData.meta = meta; nn.neuralNetworkData.isMetadataReady = true;
  const res = await new Promise((ok, bad) => nn.predictMultiple(job.feat, (e, r) => (e ? bad(e) : ok(r))));
  const rows = res.map(r => (Array.isArray(r) ? r[0] : r));
  fs.writeFileSync(process.argv[3], JSON.stringify({ value: rows.map(r => r.value), unnormalised_from: rows.map(r => r.unNormalizedValue),
                                                     meta_outputs: meta.outputs }));
}

main().catch(e => { console.error(e); process.exit(1); });
