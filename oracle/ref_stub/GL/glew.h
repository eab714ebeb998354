/* Stand-in for <GL/glew.h>, for building the reference's core translation units into oracle/_ref/ref_core
 * (oracle/Makefile, oracle/REFERENCE_PINS.md).  globals.hpp and voxel_allocator.hpp name a few GL types, constants and
 * calls in inline functions that upload buffers and report GL errors; ref_core has no GL context and never calls them.
 * The types are the ones the OpenGL registry defines; every call is a no-op. */
#ifndef REF_STUB_GLEW_H
#define REF_STUB_GLEW_H

#include <stddef.h>

typedef unsigned int GLuint;
typedef int GLint;
typedef int GLsizei;
typedef unsigned int GLenum;
typedef char GLchar;
typedef ptrdiff_t GLsizeiptr;
typedef ptrdiff_t GLintptr;

#define GL_NO_ERROR 0
#define GL_INFO_LOG_LENGTH 0x8B84
#define GL_DYNAMIC_DRAW 0x88E8
#define GL_SHADER_STORAGE_BUFFER 0x90D2

inline GLenum glGetError() { return GL_NO_ERROR; }
inline void glGetProgramiv(GLuint, GLenum, GLint* v) { *v = 1; }
inline void glGetProgramInfoLog(GLuint, GLsizei, GLsizei* n, GLchar* log) { *n = 0; *log = 0; }
inline void glGenBuffers(GLsizei, GLuint* b) { *b = 0; }
inline void glBindBuffer(GLenum, GLuint) {}
inline void glBindBufferBase(GLenum, GLuint, GLuint) {}
inline void glBufferData(GLenum, GLsizeiptr, const void*, GLenum) {}
inline void glBufferSubData(GLenum, GLintptr, GLsizeiptr, const void*) {}

#endif
