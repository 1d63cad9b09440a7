// OpenCV stand-in: everything is in cv.h
#include "cv.h"
