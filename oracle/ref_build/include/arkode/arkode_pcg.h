/* Stand-in for <arkode/arkode_pcg.h>: the reference programs include it and never attach a linear solver. */
#pragma once
