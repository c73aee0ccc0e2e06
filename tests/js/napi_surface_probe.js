// napi_surface_probe.js — the addon's observable surface without a device, for tests/test_napi_surface.py and tests/golden/gen/make_napi_surface.js.
// usage: node napi_surface_probe.js [addon.node]  -> JSON on stdout
//   out = {exports: sorted names, calls: {name: {none, objects, numbers, nulls}}}; every export but `create` is called with no argument, six {},
//   the numbers 1 .. 6 and four nulls, and each call is recorded as [how it ended, what]: ['TypeError' | 'Error' | ..., the full message],
//   ['returned', the value's kind] or ['rejected', the string]
'use strict';
const path = require('path');

const ARGS = {
  none: () => [],
  objects: () => [{}, {}, {}, {}, {}, {}],
  numbers: () => [1, 2, 3, 4, 5, 6],
  nulls: () => [null, null, null, null],
};
const kind_of = (v) => (v === null ? 'null' : typeof v !== 'object' ? typeof v : v.constructor ? v.constructor.name : 'object');

async function one(fn, args) {
  let v;
  try { v = fn(...args); } catch (e) { return [e && e.constructor ? e.constructor.name : typeof e, String(e && e.message !== undefined ? e.message : e)]; }
  if (!(v instanceof Promise)) return ['returned', kind_of(v)];
  try { return ['returned', 'Promise of ' + kind_of(await v)]; } catch (e) { return ['rejected', String(e)]; }
}

async function probe(addon) {
  const nat = require(addon);
  const out = { exports: Object.keys(nat).sort(), calls: {} };
  for (const name of out.exports) {
    if (name === 'create') continue;
    out.calls[name] = {};
    for (const set of Object.keys(ARGS)) out.calls[name][set] = await one(nat[name], ARGS[set]());
  }
  return out;
}

module.exports = { probe };
if (require.main === module) {
  const addon = path.resolve(process.argv[2] || path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'lib', 'wsa_napi.node'));
  probe(addon).then((out) => process.stdout.write(JSON.stringify(out)), (e) => { console.error(e); process.exit(1); });
}
