// make_napi_surface.js — records tests/golden/napi_surface.json from a built addon (tests/js/napi_surface_probe.js says what is recorded).
// usage: node make_napi_surface.js path/to/wsa_napi.node     (no device needed)
'use strict';
const fs = require('fs');
const path = require('path');
const { probe } = require(path.join(__dirname, '..', '..', 'js', 'napi_surface_probe.js'));

if (!process.argv[2]) { console.error('usage: node make_napi_surface.js path/to/wsa_napi.node'); process.exit(2); }
probe(path.resolve(process.argv[2])).then((out) => {
  // one line per export, so that a changed answer shows as one changed line
  const calls = Object.keys(out.calls).map((k) => JSON.stringify(k) + ': ' + JSON.stringify(out.calls[k])).join(',\n');
  fs.writeFileSync(path.join(__dirname, '..', 'napi_surface.json'), '{"exports": ' + JSON.stringify(out.exports) + ',\n"calls": {\n' + calls + '\n}}\n');
  console.log(out.exports.length + ' exports, ' + Object.keys(out.calls).length * 4 + ' calls');
}, (e) => { console.error(e); process.exit(1); });
