# Final checks of a build on a GPU host: every GPU test, smoke, the full bench line
#   bash tools/final_check.sh <tag>   -> <tag>_{tests,smoke,bench}.log in the steps' log folder
#   (tools/gpu_steps.sh); the last line of <tag>_bench.log is the bench's JSON line
T=${1:-final}
cd "$GRAFT_REPO_ROOT"
bash tools/gpu_steps.sh \
  "${T}_tests:900:python3 -u -m pytest -q --timeout 150 --timeout-method thread tests -m gpu" \
  "${T}_smoke:200:python3 -c 'import __graft_entry__ as g; g.smoke()'" \
  "${T}_bench:400:python3 bench.py --full"
