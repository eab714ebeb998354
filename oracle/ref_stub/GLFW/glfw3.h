/* Stand-in for <GLFW/glfw3.h>: globals.hpp declares a `GLFWwindow*`; ref_core opens no window. */
#ifndef REF_STUB_GLFW3_H
#define REF_STUB_GLFW3_H

struct GLFWwindow;

#endif
