#!/bin/sh
# Stand-in for the reference's util/GoldbeterModel/SolveGoldbeterODE.py, which the Goldbeter programs popen by this name from PATH
# (with beta as its argument) and read with fscanf("[%lf] [%lf]").  It integrates nothing: it prints the two numbers it finds in
# its environment in the shape numpy prints two one-element arrays.  What this pins is how the programs parse that line.
echo "[${CRD_REF_STEADY_Z}] [${CRD_REF_STEADY_Y}]"
