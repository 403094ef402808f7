/* Stand-in for <sundials/sundials_types.h>, written from the names the reference programs use: double precision only. */
#pragma once
#define SUNDIALS_DOUBLE_PRECISION 1
typedef double realtype;
typedef int booleantype;
#define RCONST(x) x
