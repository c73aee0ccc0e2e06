// crossval.js — cross-validating the app's models on a labelled feature DB, folds by file: the Node host of specification CV-1 (DESIGN.md §3;
// webspeechanalyzer_amd/crossval.py is the same in Python; K6f and include/wsa_crossval.h are the device half, reached through the addon's
// dbEval with foldOfRow).  The app's Predict button (ref src/neuralmodel.js:410) runs a model over the rows it was trained on; here every file
// is held out once.  assignFolds and foldLabels are pure and need no device.
'use strict';

const dbstats = require('./dbstats.js');
const MAX_FOLDS = 32;                                             // WSA_CROSSVAL_MAX_FOLDS: the K models of a head are one training group

// {foldOfRow: Int32Array [n], foldOfFile: [n_files], names}: files numbered as dbstats.fileColumns numbers them; a file's group is
// groupOf(file name) (default: the file itself), groups numbered in order of first appearance, group g in fold g mod k; an explicit foldOfFile
// overrides both; a row's fold is its file's, -1 without a file (never held out, never predicted, trains every fold)
function assignFolds(samples, k, groupOf, foldOfFile) {
  k |= 0;
  if (!(k >= 2 && k <= MAX_FOLDS)) throw 'crossValidate: a cross-validation has 2 .. ' + MAX_FOLDS + ' folds, got ' + k;
  const fc = dbstats.fileColumns(samples), names = fc.names;
  let fof;
  if (foldOfFile) {
    fof = Array.from(foldOfFile, (f) => f | 0);
    if (fof.length !== names.length) throw 'crossValidate: foldOfFile has ' + fof.length + ' entries, the DB has ' + names.length + ' files';
    fof.forEach((f, i) => { if (!(f >= 0 && f < k)) throw 'crossValidate: foldOfFile[' + i + '] = ' + f + ' (' + names[i] + ') is outside 0 .. ' + (k - 1); });
  } else {
    const groups = new Map(), group = (name) => (groupOf ? groupOf(name) : name);
    for (const name of names) if (!groups.has(group(name))) groups.set(group(name), groups.size);
    if (k > groups.size) throw 'crossValidate: ' + k + ' folds for ' + groups.size + ' groups (' + names.length + ' files): a fold would hold nothing out';
    fof = names.map((name) => groups.get(group(name)) % k);
  }
  return { foldOfRow: Int32Array.from(fc.fileOfRow, (f) => (f >= 0 ? fof[f] : -1)), foldOfFile: fof, names };
}

// per row the string of categorical head `name`'s true label, null where the row has none or one outside the class list / ordinal head `name`'s
// true value, null where the row has none or one that is no number: what trainModel / trainRegression take
function headLabels(samples, name, list) {
  const known = list.map(String);
  return samples.map((s) => { const v = s.truth && s.truth[0] ? s.truth[0][name] : undefined; return v && known.indexOf(String(v)) >= 0 ? String(v) : null; });
}
function headValues(samples, name) {
  return samples.map((s) => { const v = s.truth && s.truth[1] ? s.truth[1][name] : undefined; const x = v === undefined || v === null ? NaN : Number(v); return x === x ? x : null; });
}
// fold f's labels: those of its rows replaced by null, so that the selection, the `< 10` refusal, the balancing and the ranges see training rows only
const foldLabels = (labels, foldOfRow, f) => labels.map((v, i) => (foldOfRow[i] === f ? null : v));

// host: {trainModels(jobs) -> Promise of handles, evaluate(featureDB, o) -> evaluateDB's result} (formantanalyzer.js binds both).
// o = {db, classLabels, ordinalLabels, heads: [names], k, groupOf, foldOfFile, options: the app's options JSON for every head or {head: options},
// epochs, batchSize, validationSplit, seed, perFile, keepModels, inits: {head: [per fold {kernels, biases}]}, orders: {head: [per fold Uint32Array]}
// (both replace the seeded ones, as trainModel's init / orders do)}.  Fold f of every head trains with seed + 2 f; every fold of a classifier
// gets the legend the selection gives over the whole DB.  Returns a Promise of evaluateDB's {rows, files} over the held-out predictions (written
// into the samples' `pred` pairs) plus foldOfRow, foldOfFile and folds [{files, heldOut, heads: {head: {history}}}]; keepModels adds models
// {head: [handle per fold]}.
function crossValidate(host, featureDB, o) {
  const samples = featureDB.samples(o.db), hd = dbstats.heads(o.classLabels, o.ordinalLabels), names = (o.heads || []).slice();
  if (!samples.length) throw 'crossValidate: a feature DB has at least one row';
  for (const name of names)
    if (!hd.cats.some((c) => c.name === name) && hd.ords.indexOf(name) < 0) throw 'crossValidate: heads names ' + name + '; the settings have ' + hd.cats.map((c) => c.name).concat(hd.ords);
  const folds = assignFolds(samples, o.k, o.groupOf, o.foldOfFile), K = o.k | 0, seed = o.seed | 0;
  const features = samples.map((s) => Array.from(s.vector, Number));
  const tm = require('./trainmodel.js');
  const jobs = [];
  for (const name of names) {
    const cat = hd.cats.find((c) => c.name === name);
    const options = o.options && (o.options[name] || (o.options.layers ? o.options : undefined));
    const labels = cat ? headLabels(samples, name, cat.list) : headValues(samples, name);
    const legend = cat ? tm.select(labels, cat.list).legend : null;
    for (let f = 0; f < K; f++) {
      const common = { options, epochs: o.epochs, batchSize: o.batchSize, validationSplit: o.validationSplit, seed: seed + 2 * f,
        init: o.inits && o.inits[name] ? o.inits[name][f] : undefined, orders: o.orders && o.orders[name] ? o.orders[name][f] : undefined };
      try {                                                       // the selection runs here once, so that a refusal names the fold
        if (cat) tm.select(foldLabels(labels, folds.foldOfRow, f), cat.list); else tm.selectOrdinal(foldLabels(labels, folds.foldOfRow, f));
      } catch (e) { throw 'crossValidate: fold ' + f + ': ' + e; }
      jobs.push(cat ? Object.assign(common, { features, labels: foldLabels(labels, folds.foldOfRow, f), classes: cat.list, legend })
        : Object.assign(common, { regression: true, features, values: foldLabels(labels, folds.foldOfRow, f) }));
    }
  }
  return host.trainModels(jobs).then((handles) => {
    const models = {};
    names.forEach((name, i) => { models[name] = handles.slice(i * K, (i + 1) * K); });
    const out = host.evaluate(featureDB, { db: o.db, classLabels: o.classLabels, ordinalLabels: o.ordinalLabels, models, perFile: o.perFile,
      foldOfRow: folds.foldOfRow, nFolds: K });
    out.foldOfRow = folds.foldOfRow; out.foldOfFile = folds.foldOfFile;
    out.folds = [];
    for (let f = 0; f < K; f++) {
      const heads = {};
      names.forEach((name) => { heads[name] = { history: models[name][f].history }; });
      out.folds.push({ files: folds.names.filter((_, i) => folds.foldOfFile[i] === f), heldOut: folds.foldOfRow.reduce((a, g) => a + (g === f ? 1 : 0), 0), heads });
    }
    if (o.keepModels) out.models = models;
    return out;
  });
}

module.exports = { assignFolds, headLabels, headValues, foldLabels, crossValidate, MAX_FOLDS };
