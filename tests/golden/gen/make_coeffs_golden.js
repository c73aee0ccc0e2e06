// make_coeffs_golden.js — fixture generator helper for output level 12's polynomial fits (K5).  TEST INFRASTRUCTURE, build-container only.
//
// Loads the reference's formant module out of dist/main.js AT RUN TIME by ref_driver.js's recipe (slice the inner bundle, expose its webpack
// require, shim window / document; nothing of the bundle is copied into this repository) and calls its own exported
// make_coeffs([ci, frames_per_syllable, sums_per_syllable]) once per case, ONE syllable per call: make_coeffs swallows what numeric throws
// (`catch (e) { console.error(e) }`) and returns the rows collected so far, so a call that returns no row threw.
//
// usage: node make_coeffs_golden.js job.json out.json
//   job.json = {"bundle": ".../dist/main.js", "cases": [{"name", "fr": [[9 numbers] per frame], "sums": [[3 numbers] per frame]}]}
//   out.json = {"node", "cases": [{"name", "row": [23 f64 as big-endian hex] | null, "threw": message | null}]}
'use strict';
const fs = require('fs');

function load_reference(bundle_path) {
  const b = fs.readFileSync(bundle_path);
  let src = b.slice(100, 114174).toString('latin1');
  src = src.slice(src.indexOf('function(module)'));
  if (src.indexOf('n(n.s=1)') < 0) throw new Error('bundle layout changed');
  src = src.replace('n(n.s=1)', '(globalThis.__fa_require=n,n(n.s=1))');
  global.window = { setTimeout: setTimeout, screen: {} };
  global.document = { getElementById: () => ({}) };
  const mod = { exports: {} };
  (0, eval)('(' + src + ')')(mod);
  return globalThis.__fa_require(4);
}

function main() {
  const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
  const fm = load_reference(job.bundle);
  if (typeof fm.make_coeffs !== 'function') throw new Error('make_coeffs is not exported');
  const buf = Buffer.alloc(8);
  const hex = x => { buf.writeDoubleBE(x); return buf.toString('hex'); };
  const cases = [];
  for (const c of job.cases) {
    const fr = c.fr.map(r => Float32Array.from(r)), sums = c.sums.map(r => Float32Array.from(r));
    let said = null;
    const err = console.error; console.error = e => { said = String(e && e.message ? e.message : e); };
    let rows;
    try { rows = fm.make_coeffs([[[0, fr.length]], [fr], [sums]]); } finally { console.error = err; }
    if (rows.length === 1 && said === null) {
      if (rows[0].length !== 23) throw new Error(c.name + ': ' + rows[0].length + ' numbers');
      cases.push({ name: c.name, row: Array.from(rows[0], hex), threw: null });
    } else if (rows.length === 0 && said !== null) cases.push({ name: c.name, row: null, threw: said });
    else throw new Error(c.name + ': ' + rows.length + ' rows, message ' + said);
  }
  fs.writeFileSync(process.argv[3], JSON.stringify({ node: process.version, cases }));
}
main();
