// Feeds a list of level-11 callbacks, in order, to the collector of js/featuredb.js (part "0", as the app files every utterance
// result: ref src/index.js:38-44) and prints what the DB holds afterwards.  tests/test_stream_featdb_host.py compares the device DB's
// restatement (tests/stream_featdb_ref.py) against it.  argv[2]: a JSON file [[file, [t0, td], vector], ...]
'use strict';
const fs = require('fs');
const path = require('path');
const { FeatureDB } = require(path.join(__dirname, '..', '..', 'webspeechanalyzer_amd', 'js', 'featuredb.js'));

const calls = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const db = new FeatureDB();
const collect = db.collector(11, 'live');
let si = 0;
for (const [file, time, vector] of calls) collect(si++, [file], time, vector);
process.stdout.write(JSON.stringify({ refused: db.refused, samples: db.samples('live').map((s) => ({ file: s.file, seg: s.part, features: s.vector })) }));
