'use strict';
// The shared half of every case driver in this directory (`node <driver> cases.json out.json`, started by
// tests/js_host.py's run_cases): the JS host under test, the input conversion the case lists name, and the loop.
const fs = require('fs');
const path = require('path');
const p = require(path.join(__dirname, '..', '..', 'pragma-dsp_amd', 'js'));

// typed = 'f32' hands an array in as Float32Array, 'f64' as Float64Array, anything else as the plain array it is
const conv = (a, typed) => (typed === 'f32' ? Float32Array.from(a) : typed === 'f64' ? Float64Array.from(a) : a);

// runCases(handler, tail): reads the case list, writes handler(case) for each case in order -- {error: message} where
// it throws -- and then the entries of `tail` (most drivers append the root's Object.keys)
function runCases(handler, tail) {
  const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
  const out = cases.map((c) => {
    try {
      return handler(c);
    } catch (e) {
      return { error: e.message };
    }
  });
  fs.writeFileSync(process.argv[3], JSON.stringify(out.concat(tail || [])));
}

module.exports = { p, conv, runCases };
