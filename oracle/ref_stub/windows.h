/* Stand-in for the Win32 header of this name: the reference core uses nothing from it. */
