/* Stand-in for <sundials/sundials_math.h>: the reference programs include it and use none of its macros. */
#pragma once
