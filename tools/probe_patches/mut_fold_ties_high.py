# Mutant (wrong results on purpose, tests/test_gpu_fold.py must notice): the
# chain's increment table flags ties only at binades below 0, so a tying qual
# at S >= 1 is added as its rounded increment whatever the parity of S / u
import sys
d = sys.argv[1]
p = d + "/bqsr_fold.hip"
s = open(p).read()
old = "        inc[k] = tq ? -1.0 : d;  // a tie is flagged by a negative increment"
assert s.count(old) == 1
open(p, "w").write(s.replace(old, "        inc[k] = (tq && e < 0) ? -1.0 : d;"))
