# Mutant (wrong results on purpose, tests/test_gpu_fold.py must notice): an
# event stream beyond the chain's LDS prefetch is folded 4 KB at a time through
# the scratch buffer; here every piece is the stream's first one
import sys
d = sys.argv[1]
p = d + "/bqsr_fold.hip"
s = open(p).read()
old = "scratch[i] = P.streams[G.off + o + i];"
assert s.count(old) == 1
open(p, "w").write(s.replace(old, "scratch[i] = P.streams[G.off + i];"))
